// pfhe.hpp — header-only C++17 mirror of the reference's operator interface over the C ABI
// (include/pfhe.h).  Same type names, method names and argument meaning as the Rust traits:
//   U64NttTable   — primus_ntt::NttTable for U64NttTable   (crates/primus_ntt/src/ntt/mod.rs:16-113)
//   U64DcrtTable  — primus_ntt::DcrtTable for U64DcrtTable (crates/primus_ntt/src/dcrt/mod.rs:19-135)
//   U32NttTable, U32DcrtTable — the u32 / low-q tables (ntt/prime32/table.rs, dcrt/prime32.rs)
//   RNSBase, BigUintApproxSignedBasis, DcrtGlevContext, mul_dcrt_ggsw_to (and RNSBase32, BaseConverter32, BigUintApproxSignedBasis32,
//   DcrtGlevContext32: the <u32> instantiation, u32 words in memory)
//                 — primus_rns / primus_decompose / primus_lattice entry points of the RNS
//                   gadget external product (crates/primus_lattice/src/glwe/crt.rs:200-227)
// Errors: constructors throw pfhe::Error carrying the pfhe_status (the reference returns
// Result<_, NttError>); in-place transforms throw on length mismatch where the reference
// debug_asserts.  Slices are (pointer, length-in-words) pairs, in place, like `&mut [u64]`.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
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

// What the four tables share: ownership of the handle (move only), the host slices, the monomial shortcuts and the
// device-resident forms.  F names the C functions.
template <class F>
class Table {
  public:
    using H = typename F::Handle;
    using W = typename F::Word;
    ~Table() { F::destroy(h_); }
    Table(Table &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Table(const Table &) = delete;
    Table &operator=(const Table &) = delete;

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
    const H *handle() const { return h_; }

  protected:
    Table() = default;
    H *h_ = nullptr;
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

class RNSBase {
  public:
    explicit RNSBase(const std::vector<uint64_t> &moduli, int device = 0) {
        check(pfhe_rns_create(moduli.data(), moduli.size(), device, &h_));
    }
    ~RNSBase() { pfhe_rns_destroy(h_); }
    RNSBase(const RNSBase &) = delete;
    RNSBase &operator=(const RNSBase &) = delete;
    size_t moduli_count() const { return pfhe_rns_moduli_count(h_); }
    size_t big_uint_value_len() const { return pfhe_rns_big_uint_value_len(h_); }
    std::vector<uint64_t> moduli_product() const {
        std::vector<uint64_t> q(big_uint_value_len());
        check(pfhe_rns_moduli_product(h_, q.data(), q.size()));
        return q;
    }
    void compose_multiple_values_to(const uint64_t *multi_residues, size_t len_in, uint64_t *big_uint_values,
                                    size_t len_out, size_t value_count) const {
        check(pfhe_rns_compose_multiple_values_to(h_, multi_residues, len_in, big_uint_values, len_out, value_count));
    }
    void wrapping_decompose_small_values_to(const uint64_t *small_values, size_t value_count, uint64_t *multi_residues,
                                            size_t len_out, uint64_t small_value_modulus) const {
        check(pfhe_rns_wrapping_decompose_small_values_to(h_, small_values, value_count, multi_residues, len_out,
                                                          small_value_modulus));
    }
    // RNSBase::add_wrapping_decompose_small_values_scaled / add_decompose_small_values_scaled
    // (crates/primus_rns/src/base.rs:326-416); factors = (value, quotient) per modulus
    void add_wrapping_decompose_small_values_scaled(const uint64_t *small_values, size_t value_count, uint64_t *acc,
                                                    size_t len_acc, uint64_t small_value_modulus,
                                                    const std::vector<uint64_t> &factors) const {
        if (factors.size() != 2 * moduli_count()) throw Error(PFHE_ERR_BAD_LENGTH, "expected one factor per modulus");
        check(pfhe_rns_add_wrapping_decompose_small_values_scaled(h_, small_values, value_count, acc, len_acc,
                                                                  small_value_modulus, factors.data()));
    }
    void add_decompose_small_values_scaled(const uint64_t *small_values, size_t value_count, uint64_t *acc, size_t len_acc,
                                           const std::vector<uint64_t> &factors) const {
        if (factors.size() != 2 * moduli_count()) throw Error(PFHE_ERR_BAD_LENGTH, "expected one factor per modulus");
        check(pfhe_rns_add_decompose_small_values_scaled(h_, small_values, value_count, acc, len_acc, factors.data()));
    }
    // RNSBase::decompose_big_uint_values_to (crates/primus_rns/src/base.rs:457-481)
    void decompose_big_uint_values_to(const uint64_t *big_uint_values, size_t len_in, uint64_t *multi_residues,
                                      size_t len_out, size_t value_count) const {
        check(pfhe_rns_decompose_big_uint_values_to(h_, big_uint_values, len_in, multi_residues, len_out, value_count));
    }
    const pfhe_rns *handle() const { return h_; }

  private:
    pfhe_rns *h_ = nullptr;
};

// primus_rns::BaseConverter (crates/primus_rns/src/converter.rs:21): modulus-major arrays; the reference's
// `scratch` argument has no counterpart
class BaseConverter {
  public:
    BaseConverter(const RNSBase &input_base, const RNSBase &output_base) {
        check(pfhe_conv_create(input_base.handle(), output_base.handle(), &h_));
    }
    ~BaseConverter() { pfhe_conv_destroy(h_); }
    BaseConverter(const BaseConverter &) = delete;
    BaseConverter &operator=(const BaseConverter &) = delete;
    size_t input_moduli_count() const { return pfhe_conv_input_moduli_count(h_); }
    size_t output_moduli_count() const { return pfhe_conv_output_moduli_count(h_); }
    void fast_convert_array(const uint64_t *crt_poly_in, size_t len_in, uint64_t *crt_poly_out, size_t len_out,
                            size_t poly_length) const {
        check(pfhe_conv_fast_convert_array(h_, crt_poly_in, len_in, crt_poly_out, len_out, poly_length));
    }
    void exact_convert_array(const uint64_t *crt_poly_in, size_t len_in, uint64_t *crt_poly_out, size_t len_out,
                             size_t poly_length) const {
        check(pfhe_conv_exact_convert_array(h_, crt_poly_in, len_in, crt_poly_out, len_out, poly_length));
    }
    void fast_convert_array_dev(const uint64_t *in_dev, size_t len_in, uint64_t *out_dev, size_t len_out,
                                size_t poly_length, void *stream = nullptr) const {
        check(pfhe_conv_fast_convert_array_dev(h_, in_dev, len_in, out_dev, len_out, poly_length, stream));
    }
    void exact_convert_array_dev(const uint64_t *in_dev, size_t len_in, uint64_t *out_dev, size_t len_out,
                                 size_t poly_length, void *stream = nullptr) const {
        check(pfhe_conv_exact_convert_array_dev(h_, in_dev, len_in, out_dev, len_out, poly_length, stream));
    }

  private:
    pfhe_conv *h_ = nullptr;
};

class BigUintApproxSignedBasis {
  public:
    BigUintApproxSignedBasis(const RNSBase &base, uint32_t log_basis, size_t reverse_length = 0) {
        check(pfhe_basis_create(base.handle(), log_basis, reverse_length, &h_));
    }
    ~BigUintApproxSignedBasis() { pfhe_basis_destroy(h_); }
    BigUintApproxSignedBasis(const BigUintApproxSignedBasis &) = delete;
    BigUintApproxSignedBasis &operator=(const BigUintApproxSignedBasis &) = delete;
    size_t decompose_length() const { return pfhe_basis_decompose_length(h_); }
    uint32_t log_basis() const { return pfhe_basis_log_basis(h_); }
    uint32_t drop_bits() const { return pfhe_basis_drop_bits(h_); }
    uint64_t basis_value() const { return pfhe_basis_basis_value(h_); }
    void init_value_carry_slice_inplace(uint64_t *values, size_t len, uint8_t *carries, size_t count) const {
        check(pfhe_basis_init_value_carry_slice_inplace(h_, values, len, carries, count));
    }
    void unsigned_decompose_slice_to(size_t level, const uint64_t *values, size_t len, uint64_t *digits,
                                     uint8_t *carries, size_t count) const {
        check(pfhe_basis_unsigned_decompose_slice_to(h_, level, values, len, digits, carries, count));
    }
    // decomposer_iter().nth(level).decompose_slice_to (big_integer/common.rs:289-306): signed digit as a residue mod Q
    void decompose_slice_to(size_t level, const uint64_t *values, size_t len, uint64_t *decomposed_values, size_t len_out,
                            uint8_t *carries, size_t count) const {
        check(pfhe_basis_decompose_slice_to(h_, level, values, len, decomposed_values, len_out, carries, count));
    }
    const pfhe_basis *handle() const { return h_; }

  private:
    pfhe_basis *h_ = nullptr;
};

// DcrtGlevContext (crates/primus_lattice/src/context/glev.rs:4-68) + the handles the reference
// passes next to it.  One holder at a time, like the `&mut` it mirrors: a call from a second thread while one is inside throws
// (PFHE_ERR_BUSY, "plan in use"); successive calls on different streams are ordered by the library.
class DcrtGlevContext {
  public:
    DcrtGlevContext(const U64DcrtTable &table, const RNSBase &base, const BigUintApproxSignedBasis &basis,
                    size_t glwe_dimension = 1, size_t chunk = 0) {
        check(pfhe_extprod_plan_create(table.handle(), base.handle(), basis.handle(), glwe_dimension, chunk, &h_));
    }
    ~DcrtGlevContext() { pfhe_extprod_plan_destroy(h_); }
    DcrtGlevContext(const DcrtGlevContext &) = delete;
    DcrtGlevContext &operator=(const DcrtGlevContext &) = delete;
    pfhe_extprod_plan *handle() const { return h_; }
    bool in_use() const { return pfhe_extprod_plan_in_use(h_) != 0; }  // some thread is inside a call on this context

  private:
    pfhe_extprod_plan *h_ = nullptr;
};

// CrtGlwe::mul_dcrt_ggsw_to (crates/primus_lattice/src/glwe/crt.rs:200-227), host slices
inline void mul_dcrt_ggsw_to(const uint64_t *crt_glwe, size_t len_glwe, const uint64_t *dcrt_ggsw, size_t len_ggsw,
                             uint64_t *result, size_t len_result, DcrtGlevContext &context,
                             bool into_coeff_form = false) {
    check(pfhe_extprod_mul_dcrt_ggsw_to(context.handle(), crt_glwe, len_glwe, dcrt_ggsw, len_ggsw, result, len_result,
                                        into_coeff_form));
}

// device-resident batches
inline void mul_dcrt_ggsw_to_dev(const uint64_t *crt_glwe_dev, size_t len_glwe, const uint64_t *dcrt_ggsw_dev,
                                 size_t len_ggsw, uint64_t *result_dev, size_t len_result, DcrtGlevContext &context,
                                 bool into_coeff_form = false, void *stream = nullptr) {
    check(pfhe_extprod_mul_dcrt_ggsw_to_dev(context.handle(), crt_glwe_dev, len_glwe, dcrt_ggsw_dev, len_ggsw,
                                            result_dev, len_result, into_coeff_form, stream));
}

// The batched blind rotation over the external product (pfhe_blindrot_*): for every step i and ciphertext e,
// ACC_e += coeff_form(((X^{exps[e*n_steps+i]} - 1) * ACC_e) (x) BSK_i)  — CrtGlwe::mul_monic_monomial_assign
// (glwe/crt.rs:76-114), sub_element_wise_assign, CrtGlwe::mul_dcrt_ggsw_to (glwe/crt.rs:200-227), write_coeff_form,
// add_element_wise_assign.  Owns its product plan and glue buffers; one holder at a time, like DcrtGlevContext.
class BlindRotate {
  public:
    BlindRotate(const U64DcrtTable &table, const RNSBase &base, const BigUintApproxSignedBasis &basis,
                size_t glwe_dimension = 1, size_t chunk = 0) {
        check(pfhe_blindrot_create(table.handle(), base.handle(), basis.handle(), glwe_dimension, chunk, &h_));
    }
    ~BlindRotate() { pfhe_blindrot_destroy(h_); }
    BlindRotate(const BlindRotate &) = delete;
    BlindRotate &operator=(const BlindRotate &) = delete;
    pfhe_blindrot *handle() const { return h_; }
    bool in_use() const { return pfhe_blindrot_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_blindrot_scratch_bytes(h_); }
    // host slices; every exponent below 2N
    void rotate(uint64_t *acc, size_t len_acc, const uint64_t *bsk, size_t len_bsk, const uint32_t *exps,
                size_t len_exps) {
        check(pfhe_blindrot_rotate(h_, acc, len_acc, bsk, len_bsk, exps, len_exps));
    }
    // device buffers, queued on `stream` (exponents taken modulo 2N)
    void rotate_dev(uint64_t *acc_dev, size_t len_acc, const uint64_t *bsk_dev, size_t len_bsk, const uint32_t *exps_dev,
                    size_t len_exps, void *stream = nullptr) {
        check(pfhe_blindrot_rotate_dev(h_, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream));
    }

  private:
    pfhe_blindrot *h_ = nullptr;
};

// ---- the <u32> instantiation of the same operators (RNSBase<u32>, BigUintApproxSignedBasis<u32> — the type the
// reference's tests/big_uint.rs:13 runs — and CrtGlwe<u32>::mul_dcrt_ggsw_to over a U32DcrtTable).  Words are
// uint32_t in memory (residues, digits, limbs of big integers); moduli below 2^30, log_basis below 32; up to 32 moduli.
class RNSBase32 {
  public:
    explicit RNSBase32(const std::vector<uint32_t> &moduli, int device = 0) {
        check(pfhe_rns32_create(moduli.data(), moduli.size(), device, &h_));
    }
    ~RNSBase32() { pfhe_rns32_destroy(h_); }
    RNSBase32(const RNSBase32 &) = delete;
    RNSBase32 &operator=(const RNSBase32 &) = delete;
    size_t moduli_count() const { return pfhe_rns32_moduli_count(h_); }
    size_t big_uint_value_len() const { return pfhe_rns32_big_uint_value_len(h_); }
    std::vector<uint32_t> moduli_product() const {
        std::vector<uint32_t> q(big_uint_value_len());
        check(pfhe_rns32_moduli_product(h_, q.data(), q.size()));
        return q;
    }
    void compose_multiple_values_to(const uint32_t *multi_residues, size_t len_in, uint32_t *big_uint_values,
                                    size_t len_out, size_t value_count) const {
        check(pfhe_rns32_compose_multiple_values_to(h_, multi_residues, len_in, big_uint_values, len_out, value_count));
    }
    void wrapping_decompose_small_values_to(const uint32_t *small_values, size_t value_count, uint32_t *multi_residues,
                                            size_t len_out, uint32_t small_value_modulus) const {
        check(pfhe_rns32_wrapping_decompose_small_values_to(h_, small_values, value_count, multi_residues, len_out,
                                                            small_value_modulus));
    }
    void add_wrapping_decompose_small_values_scaled(const uint32_t *small_values, size_t value_count, uint32_t *acc,
                                                    size_t len_acc, uint32_t small_value_modulus,
                                                    const std::vector<uint32_t> &factors) const {
        if (factors.size() != 2 * moduli_count()) throw Error(PFHE_ERR_BAD_LENGTH, "expected one factor per modulus");
        check(pfhe_rns32_add_wrapping_decompose_small_values_scaled(h_, small_values, value_count, acc, len_acc,
                                                                    small_value_modulus, factors.data()));
    }
    void add_decompose_small_values_scaled(const uint32_t *small_values, size_t value_count, uint32_t *acc, size_t len_acc,
                                           const std::vector<uint32_t> &factors) const {
        if (factors.size() != 2 * moduli_count()) throw Error(PFHE_ERR_BAD_LENGTH, "expected one factor per modulus");
        check(pfhe_rns32_add_decompose_small_values_scaled(h_, small_values, value_count, acc, len_acc, factors.data()));
    }
    void decompose_big_uint_values_to(const uint32_t *big_uint_values, size_t len_in, uint32_t *multi_residues,
                                      size_t len_out, size_t value_count) const {
        check(pfhe_rns32_decompose_big_uint_values_to(h_, big_uint_values, len_in, multi_residues, len_out, value_count));
    }
    const pfhe_rns32 *handle() const { return h_; }

  private:
    pfhe_rns32 *h_ = nullptr;
};

// primus_rns::BaseConverter<u32, BarrettModulus<u32>> (converter.rs:21, generic over T: FheUint)
class BaseConverter32 {
  public:
    BaseConverter32(const RNSBase32 &input_base, const RNSBase32 &output_base) {
        check(pfhe_conv32_create(input_base.handle(), output_base.handle(), &h_));
    }
    ~BaseConverter32() { pfhe_conv32_destroy(h_); }
    BaseConverter32(const BaseConverter32 &) = delete;
    BaseConverter32 &operator=(const BaseConverter32 &) = delete;
    size_t input_moduli_count() const { return pfhe_conv32_input_moduli_count(h_); }
    size_t output_moduli_count() const { return pfhe_conv32_output_moduli_count(h_); }
    void fast_convert_array(const uint32_t *crt_poly_in, size_t len_in, uint32_t *crt_poly_out, size_t len_out,
                            size_t poly_length) const {
        check(pfhe_conv32_fast_convert_array(h_, crt_poly_in, len_in, crt_poly_out, len_out, poly_length));
    }
    void exact_convert_array(const uint32_t *crt_poly_in, size_t len_in, uint32_t *crt_poly_out, size_t len_out,
                             size_t poly_length) const {
        check(pfhe_conv32_exact_convert_array(h_, crt_poly_in, len_in, crt_poly_out, len_out, poly_length));
    }
    void fast_convert_array_dev(const uint32_t *in_dev, size_t len_in, uint32_t *out_dev, size_t len_out,
                                size_t poly_length, void *stream = nullptr) const {
        check(pfhe_conv32_fast_convert_array_dev(h_, in_dev, len_in, out_dev, len_out, poly_length, stream));
    }
    void exact_convert_array_dev(const uint32_t *in_dev, size_t len_in, uint32_t *out_dev, size_t len_out,
                                 size_t poly_length, void *stream = nullptr) const {
        check(pfhe_conv32_exact_convert_array_dev(h_, in_dev, len_in, out_dev, len_out, poly_length, stream));
    }

  private:
    pfhe_conv32 *h_ = nullptr;
};

class BigUintApproxSignedBasis32 {
  public:
    BigUintApproxSignedBasis32(const RNSBase32 &base, uint32_t log_basis, size_t reverse_length = 0) {
        check(pfhe_basis32_create(base.handle(), log_basis, reverse_length, &h_));
    }
    ~BigUintApproxSignedBasis32() { pfhe_basis32_destroy(h_); }
    BigUintApproxSignedBasis32(const BigUintApproxSignedBasis32 &) = delete;
    BigUintApproxSignedBasis32 &operator=(const BigUintApproxSignedBasis32 &) = delete;
    size_t decompose_length() const { return pfhe_basis32_decompose_length(h_); }
    uint32_t log_basis() const { return pfhe_basis32_log_basis(h_); }
    uint32_t drop_bits() const { return pfhe_basis32_drop_bits(h_); }
    uint32_t basis_value() const { return pfhe_basis32_basis_value(h_); }
    void init_value_carry_slice_inplace(uint32_t *values, size_t len, uint8_t *carries, size_t count) const {
        check(pfhe_basis32_init_value_carry_slice_inplace(h_, values, len, carries, count));
    }
    void unsigned_decompose_slice_to(size_t level, const uint32_t *values, size_t len, uint32_t *digits,
                                     uint8_t *carries, size_t count) const {
        check(pfhe_basis32_unsigned_decompose_slice_to(h_, level, values, len, digits, carries, count));
    }
    void decompose_slice_to(size_t level, const uint32_t *values, size_t len, uint32_t *decomposed_values, size_t len_out,
                            uint8_t *carries, size_t count) const {
        check(pfhe_basis32_decompose_slice_to(h_, level, values, len, decomposed_values, len_out, carries, count));
    }
    const pfhe_basis32 *handle() const { return h_; }

  private:
    pfhe_basis32 *h_ = nullptr;
};

// DcrtGlevContext over a U32DcrtTable; one holder at a time like DcrtGlevContext
class DcrtGlevContext32 {
  public:
    DcrtGlevContext32(const U32DcrtTable &table, const RNSBase32 &base, const BigUintApproxSignedBasis32 &basis,
                      size_t glwe_dimension = 1, size_t chunk = 0) {
        check(pfhe_extprod32_plan_create(table.handle(), base.handle(), basis.handle(), glwe_dimension, chunk, &h_));
    }
    ~DcrtGlevContext32() { pfhe_extprod32_plan_destroy(h_); }
    DcrtGlevContext32(const DcrtGlevContext32 &) = delete;
    DcrtGlevContext32 &operator=(const DcrtGlevContext32 &) = delete;
    pfhe_extprod32_plan *handle() const { return h_; }
    bool in_use() const { return pfhe_extprod32_plan_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_extprod32_plan_scratch_bytes(h_); }

  private:
    pfhe_extprod32_plan *h_ = nullptr;
};

// the batched blind rotation over the u32 product, as BlindRotate
class BlindRotate32 {
  public:
    BlindRotate32(const U32DcrtTable &table, const RNSBase32 &base, const BigUintApproxSignedBasis32 &basis,
                  size_t glwe_dimension = 1, size_t chunk = 0) {
        check(pfhe_blindrot32_create(table.handle(), base.handle(), basis.handle(), glwe_dimension, chunk, &h_));
    }
    ~BlindRotate32() { pfhe_blindrot32_destroy(h_); }
    BlindRotate32(const BlindRotate32 &) = delete;
    BlindRotate32 &operator=(const BlindRotate32 &) = delete;
    pfhe_blindrot32 *handle() const { return h_; }
    bool in_use() const { return pfhe_blindrot32_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_blindrot32_scratch_bytes(h_); }
    void rotate(uint32_t *acc, size_t len_acc, const uint32_t *bsk, size_t len_bsk, const uint32_t *exps,
                size_t len_exps) {
        check(pfhe_blindrot32_rotate(h_, acc, len_acc, bsk, len_bsk, exps, len_exps));
    }
    void rotate_dev(uint32_t *acc_dev, size_t len_acc, const uint32_t *bsk_dev, size_t len_bsk, const uint32_t *exps_dev,
                    size_t len_exps, void *stream = nullptr) {
        check(pfhe_blindrot32_rotate_dev(h_, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream));
    }

  private:
    pfhe_blindrot32 *h_ = nullptr;
};

// CrtGlwe<u32>::mul_dcrt_ggsw_to (crates/primus_lattice/src/glwe/crt.rs:200-227)
inline void mul_dcrt_ggsw_to(const uint32_t *crt_glwe, size_t len_glwe, const uint32_t *dcrt_ggsw, size_t len_ggsw,
                             uint32_t *result, size_t len_result, DcrtGlevContext32 &context,
                             bool into_coeff_form = false) {
    check(pfhe_extprod32_mul_dcrt_ggsw_to(context.handle(), crt_glwe, len_glwe, dcrt_ggsw, len_ggsw, result, len_result,
                                          into_coeff_form));
}

inline void mul_dcrt_ggsw_to_dev(const uint32_t *crt_glwe_dev, size_t len_glwe, const uint32_t *dcrt_ggsw_dev,
                                 size_t len_ggsw, uint32_t *result_dev, size_t len_result, DcrtGlevContext32 &context,
                                 bool into_coeff_form = false, void *stream = nullptr) {
    check(pfhe_extprod32_mul_dcrt_ggsw_to_dev(context.handle(), crt_glwe_dev, len_glwe, dcrt_ggsw_dev, len_ggsw,
                                              result_dev, len_result, into_coeff_form, stream));
}

// FullComplex64FftTable — primus_fft::FftTable (crates/primus_fft/src/table.rs, complex64/table.rs:47-130): Fourier
// values as interleaved (re, im) doubles, N complex values per polynomial; lengths count complex values / torus words.
class FullComplex64FftTable {
  public:
    explicit FullComplex64FftTable(uint32_t log_n, int device = 0) { check(pfhe_fft_create(log_n, device, &h_)); }
    ~FullComplex64FftTable() { pfhe_fft_destroy(h_); }
    FullComplex64FftTable(const FullComplex64FftTable &) = delete;
    FullComplex64FftTable &operator=(const FullComplex64FftTable &) = delete;
    pfhe_fft *handle() const { return h_; }
    size_t poly_length() const { return pfhe_fft_poly_length(h_); }
    size_t fourier_length() const { return pfhe_fft_fourier_length(h_); }
    void forward_torus_slice(const uint64_t *in, size_t len_in, double *out, size_t len_out) const {
        check(pfhe_fft_forward_torus_slice(h_, in, len_in, out, len_out));
    }
    void forward_torus_slice(const uint32_t *in, size_t len_in, double *out, size_t len_out) const {
        check(pfhe_fft_forward_torus32_slice(h_, in, len_in, out, len_out));
    }
    void inverse_torus_slice(const double *in, size_t len_in, uint64_t *out, size_t len_out) const {
        check(pfhe_fft_inverse_torus_slice(h_, in, len_in, out, len_out));
    }
    void inverse_torus_slice(const double *in, size_t len_in, uint32_t *out, size_t len_out) const {
        check(pfhe_fft_inverse_torus32_slice(h_, in, len_in, out, len_out));
    }
    void forward_torus_dev(const uint64_t *in, size_t len_in, double *out, size_t len_out, void *stream = nullptr) const {
        check(pfhe_fft_forward_torus_dev(h_, in, len_in, out, len_out, stream));
    }
    void forward_torus_dev(const uint32_t *in, size_t len_in, double *out, size_t len_out, void *stream = nullptr) const {
        check(pfhe_fft_forward_torus32_dev(h_, in, len_in, out, len_out, stream));
    }
    void inverse_torus_dev(const double *in, size_t len_in, uint64_t *out, size_t len_out, void *stream = nullptr) const {
        check(pfhe_fft_inverse_torus_dev(h_, in, len_in, out, len_out, stream));
    }
    void inverse_torus_dev(const double *in, size_t len_in, uint32_t *out, size_t len_out, void *stream = nullptr) const {
        check(pfhe_fft_inverse_torus32_dev(h_, in, len_in, out, len_out, stream));
    }

  private:
    pfhe_fft *h_ = nullptr;
};

// TfheFftContext<u64> with its power-of-two ApproxSignedBasis<u64> (primus_lattice/src/context/tfhe.rs,
// primus_decompose/src/primitive/basis.rs:47-177); decompose_length 0 = the full 64 / log_basis.  One holder at a time.
class TfheFftContext {
  public:
    TfheFftContext(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis,
                   size_t decompose_length = 0, size_t chunk = 0) {
        check(pfhe_tfhe_plan_create(fft.handle(), glwe_dimension, log_basis, decompose_length, chunk, &h_));
    }
    ~TfheFftContext() { pfhe_tfhe_plan_destroy(h_); }
    TfheFftContext(const TfheFftContext &) = delete;
    TfheFftContext &operator=(const TfheFftContext &) = delete;
    pfhe_tfhe_plan *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe_plan_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe_plan_scratch_bytes(h_); }

  private:
    pfhe_tfhe_plan *h_ = nullptr;
};

// the u32 torus
class TfheFftContext32 {
  public:
    TfheFftContext32(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis,
                     size_t decompose_length = 0, size_t chunk = 0) {
        check(pfhe_tfhe32_plan_create(fft.handle(), glwe_dimension, log_basis, decompose_length, chunk, &h_));
    }
    ~TfheFftContext32() { pfhe_tfhe32_plan_destroy(h_); }
    TfheFftContext32(const TfheFftContext32 &) = delete;
    TfheFftContext32 &operator=(const TfheFftContext32 &) = delete;
    pfhe_tfhe32_plan *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe32_plan_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe32_plan_scratch_bytes(h_); }

  private:
    pfhe_tfhe32_plan *h_ = nullptr;
};

// external_product_to (crates/primus_lattice/src/tfhe/external_product.rs:36-93): a batch of GLWE ciphertexts, one
// Fourier GGSW key (len_key complex values)
inline void external_product_to(const uint64_t *input, size_t len_input, const double *key, size_t len_key, uint64_t *output,
                                size_t len_output, TfheFftContext &context) {
    check(pfhe_tfhe_external_product_to(context.handle(), input, len_input, key, len_key, output, len_output));
}
inline void external_product_to(const uint32_t *input, size_t len_input, const double *key, size_t len_key, uint32_t *output,
                                size_t len_output, TfheFftContext32 &context) {
    check(pfhe_tfhe32_external_product_to(context.handle(), input, len_input, key, len_key, output, len_output));
}
inline void external_product_to_dev(const uint64_t *input_dev, size_t len_input, const double *key_dev, size_t len_key,
                                    uint64_t *output_dev, size_t len_output, TfheFftContext &context, void *stream = nullptr) {
    check(pfhe_tfhe_external_product_to_dev(context.handle(), input_dev, len_input, key_dev, len_key, output_dev, len_output,
                                            stream));
}
inline void external_product_to_dev(const uint32_t *input_dev, size_t len_input, const double *key_dev, size_t len_key,
                                    uint32_t *output_dev, size_t len_output, TfheFftContext32 &context,
                                    void *stream = nullptr) {
    check(pfhe_tfhe32_external_product_to_dev(context.handle(), input_dev, len_input, key_dev, len_key, output_dev,
                                              len_output, stream));
}

// The batched blind rotation over the TFHE product (pfhe_tfhe_blindrot_*): for every step i and ciphertext e,
// ACC_e += external_product_to(X^{exps[e*n_steps+i]} * ACC_e - ACC_e, BSK_i) on torus words (the rotation of
// CrtGlwe::mul_monic_monomial_assign, glwe/crt.rs:76-114; external_product_to, tfhe/external_product.rs:36-93).  Takes
// TfheFftContext's arguments, owns its product plan and glue buffers; one holder at a time.
class TfheBlindRotate {
  public:
    TfheBlindRotate(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length = 0,
                    size_t chunk = 0) {
        check(pfhe_tfhe_blindrot_create(fft.handle(), glwe_dimension, log_basis, decompose_length, chunk, &h_));
    }
    ~TfheBlindRotate() { pfhe_tfhe_blindrot_destroy(h_); }
    TfheBlindRotate(const TfheBlindRotate &) = delete;
    TfheBlindRotate &operator=(const TfheBlindRotate &) = delete;
    pfhe_tfhe_blindrot *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe_blindrot_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe_blindrot_scratch_bytes(h_); }
    // host slices; every exponent below 2N
    void rotate(uint64_t *acc, size_t len_acc, const double *bsk, size_t len_bsk, const uint32_t *exps, size_t len_exps) {
        check(pfhe_tfhe_blindrot_rotate(h_, acc, len_acc, bsk, len_bsk, exps, len_exps));
    }
    // device buffers, queued on `stream` (exponents taken modulo 2N)
    void rotate_dev(uint64_t *acc_dev, size_t len_acc, const double *bsk_dev, size_t len_bsk, const uint32_t *exps_dev,
                    size_t len_exps, void *stream = nullptr) {
        check(pfhe_tfhe_blindrot_rotate_dev(h_, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream));
    }

  private:
    pfhe_tfhe_blindrot *h_ = nullptr;
};

// the same over the u32 torus
class TfheBlindRotate32 {
  public:
    TfheBlindRotate32(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length = 0,
                      size_t chunk = 0) {
        check(pfhe_tfhe32_blindrot_create(fft.handle(), glwe_dimension, log_basis, decompose_length, chunk, &h_));
    }
    ~TfheBlindRotate32() { pfhe_tfhe32_blindrot_destroy(h_); }
    TfheBlindRotate32(const TfheBlindRotate32 &) = delete;
    TfheBlindRotate32 &operator=(const TfheBlindRotate32 &) = delete;
    pfhe_tfhe32_blindrot *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe32_blindrot_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe32_blindrot_scratch_bytes(h_); }
    // host slices; every exponent below 2N
    void rotate(uint32_t *acc, size_t len_acc, const double *bsk, size_t len_bsk, const uint32_t *exps, size_t len_exps) {
        check(pfhe_tfhe32_blindrot_rotate(h_, acc, len_acc, bsk, len_bsk, exps, len_exps));
    }
    // device buffers, queued on `stream` (exponents taken modulo 2N)
    void rotate_dev(uint32_t *acc_dev, size_t len_acc, const double *bsk_dev, size_t len_bsk, const uint32_t *exps_dev,
                    size_t len_exps, void *stream = nullptr) {
        check(pfhe_tfhe32_blindrot_rotate_dev(h_, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream));
    }

  private:
    pfhe_tfhe32_blindrot *h_ = nullptr;
};

// The multi-bit blind rotation (pfhe_tfhe_mbrot_*): the mask is consumed grouping_factor (1..4) elements at a time; for every
// group t and ciphertext e, ACC_e = external_product_to(ACC_e, sum_j X^{r_j} * BSK[t][j]) with r_j the subset sum of the
// group's exponents at the set bits of j.  Binary LWE keys; bsk is groups x 2^g Fourier GGSW keys.  Owns the scratch of its
// form; one holder at a time.  TfheMultiBitBlindRotate32: the u32 torus.
class TfheMultiBitBlindRotate {
  public:
    TfheMultiBitBlindRotate(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                            size_t grouping_factor, size_t chunk = 0) {
        check(pfhe_tfhe_mbrot_create(fft.handle(), glwe_dimension, log_basis, decompose_length, grouping_factor, chunk, &h_));
    }
    ~TfheMultiBitBlindRotate() { pfhe_tfhe_mbrot_destroy(h_); }
    TfheMultiBitBlindRotate(const TfheMultiBitBlindRotate &) = delete;
    TfheMultiBitBlindRotate &operator=(const TfheMultiBitBlindRotate &) = delete;
    pfhe_tfhe_mbrot *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe_mbrot_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe_mbrot_scratch_bytes(h_); }
    // host slices; every exponent below 2N
    void rotate(uint64_t *acc, size_t len_acc, const double *bsk, size_t len_bsk, const uint32_t *exps, size_t len_exps) {
        check(pfhe_tfhe_mbrot_rotate(h_, acc, len_acc, bsk, len_bsk, exps, len_exps));
    }
    // device buffers, queued on `stream` (exponents taken modulo 2N)
    void rotate_dev(uint64_t *acc_dev, size_t len_acc, const double *bsk_dev, size_t len_bsk, const uint32_t *exps_dev,
                    size_t len_exps, void *stream = nullptr) {
        check(pfhe_tfhe_mbrot_rotate_dev(h_, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream));
    }

  private:
    pfhe_tfhe_mbrot *h_ = nullptr;
};

class TfheMultiBitBlindRotate32 {
  public:
    TfheMultiBitBlindRotate32(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                              size_t grouping_factor, size_t chunk = 0) {
        check(pfhe_tfhe32_mbrot_create(fft.handle(), glwe_dimension, log_basis, decompose_length, grouping_factor, chunk, &h_));
    }
    ~TfheMultiBitBlindRotate32() { pfhe_tfhe32_mbrot_destroy(h_); }
    TfheMultiBitBlindRotate32(const TfheMultiBitBlindRotate32 &) = delete;
    TfheMultiBitBlindRotate32 &operator=(const TfheMultiBitBlindRotate32 &) = delete;
    pfhe_tfhe32_mbrot *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe32_mbrot_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe32_mbrot_scratch_bytes(h_); }
    // host slices; every exponent below 2N
    void rotate(uint32_t *acc, size_t len_acc, const double *bsk, size_t len_bsk, const uint32_t *exps, size_t len_exps) {
        check(pfhe_tfhe32_mbrot_rotate(h_, acc, len_acc, bsk, len_bsk, exps, len_exps));
    }
    // device buffers, queued on `stream` (exponents taken modulo 2N)
    void rotate_dev(uint32_t *acc_dev, size_t len_acc, const double *bsk_dev, size_t len_bsk, const uint32_t *exps_dev,
                    size_t len_exps, void *stream = nullptr) {
        check(pfhe_tfhe32_mbrot_rotate_dev(h_, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream));
    }

  private:
    pfhe_tfhe32_mbrot *h_ = nullptr;
};

// the combined key of one ciphertext and one group as a key in the reference's layout (pfhe_tfhe_mb_combine_key_dev)
inline void tfhe_multibit_combine_key_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, size_t decompose_length,
                                          size_t grouping_factor, const double *keys_dev, size_t len_keys,
                                          const uint32_t *exps_dev, size_t len_exps, double *out_dev, size_t len_out,
                                          void *stream = nullptr) {
    check(pfhe_tfhe_mb_combine_key_dev(fft.handle(), glwe_dimension, decompose_length, grouping_factor, keys_dev, len_keys,
                                       exps_dev, len_exps, out_dev, len_out, stream));
}

// X^{exps[e]} * element e for elements of polys_per_exp torus polynomials (the X^{-b_e} * TV that starts a bootstrap)
inline void mul_monomial_each_to_dev(const FullComplex64FftTable &fft, const uint64_t *a_dev, size_t len,
                                     const uint32_t *exps_dev, size_t polys_per_exp, uint64_t *out_dev,
                                     void *stream = nullptr) {
    check(pfhe_tfhe_mul_monomial_each_to_dev(fft.handle(), a_dev, len, exps_dev, polys_per_exp, out_dev, stream));
}
inline void mul_monomial_each_to_dev(const FullComplex64FftTable &fft, const uint32_t *a_dev, size_t len,
                                     const uint32_t *exps_dev, size_t polys_per_exp, uint32_t *out_dev,
                                     void *stream = nullptr) {
    check(pfhe_tfhe32_mul_monomial_each_to_dev(fft.handle(), a_dev, len, exps_dev, polys_per_exp, out_dev, stream));
}

// The project's own modulus switch (the reference has none): exps[e*n + i] = sw(a_{e,i}), neg_b[e] = (2N - sw(b_e)) mod 2N
inline void lwe_modulus_switch_dev(int device, const uint64_t *lwe_dev, size_t len_lwe, size_t lwe_dimension, uint32_t log_n,
                                   uint32_t *exps_dev, size_t len_exps, uint32_t *neg_b_dev, size_t len_neg_b,
                                   void *stream = nullptr) {
    check(pfhe_tfhe_modswitch_dev(device, lwe_dev, len_lwe, lwe_dimension, log_n, exps_dev, len_exps, neg_b_dev, len_neg_b,
                                  stream));
}
// ... to multiples of 2^log_stride (log_stride <= log_n), what a many-LUT rotation takes; log_stride 0 is the call above
inline void lwe_modulus_switch_strided_dev(int device, const uint64_t *lwe_dev, size_t len_lwe, size_t lwe_dimension,
                                           uint32_t log_n, uint32_t log_stride, uint32_t *exps_dev, size_t len_exps,
                                           uint32_t *neg_b_dev, size_t len_neg_b, void *stream = nullptr) {
    check(pfhe_tfhe_modswitch_stride_dev(device, lwe_dev, len_lwe, lwe_dimension, log_n, log_stride, exps_dev, len_exps,
                                         neg_b_dev, len_neg_b, stream));
}
// Rlwe::extract_lwe_with_index (primus_lattice/src/rlwe/coeff.rs:194-227) per mask polynomial of a GLWE ciphertext
inline void glwe_sample_extract(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint64_t *glwe, size_t len_glwe,
                                size_t index, uint64_t *lwe, size_t len_lwe) {
    check(pfhe_tfhe_sample_extract(fft.handle(), glwe_dimension, glwe, len_glwe, index, lwe, len_lwe));
}
inline void glwe_sample_extract_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint64_t *glwe_dev,
                                    size_t len_glwe, size_t index, uint64_t *lwe_dev, size_t len_lwe, void *stream = nullptr) {
    check(pfhe_tfhe_sample_extract_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, index, lwe_dev, len_lwe, stream));
}
// LWE key switch: out = (0, b) - sum_i sum_j d_{i,j} * KSK[i][j] (Lwe::add_mul_scalar_assign, lwe/single_message.rs:262-268,
// with ApproxSignedBasis's digits); decompose_length 0 = the full BITS / log_basis
inline void lwe_keyswitch(int device, const uint64_t *lwe_in, size_t len_in, size_t in_dimension, const uint64_t *ksk, size_t len_ksk,
                          size_t out_dimension, uint32_t log_basis, size_t decompose_length, uint64_t *lwe_out, size_t len_out) {
    check(pfhe_tfhe_keyswitch(device, lwe_in, len_in, in_dimension, ksk, len_ksk, out_dimension, log_basis, decompose_length,
                              lwe_out, len_out));
}
inline void lwe_keyswitch_dev(int device, const uint64_t *lwe_in_dev, size_t len_in, size_t in_dimension, const uint64_t *ksk_dev,
                              size_t len_ksk, size_t out_dimension, uint32_t log_basis, size_t decompose_length,
                              uint64_t *lwe_out_dev, size_t len_out, void *stream = nullptr) {
    check(pfhe_tfhe_keyswitch_dev(device, lwe_in_dev, len_in, in_dimension, ksk_dev, len_ksk, out_dimension, log_basis,
                                  decompose_length, lwe_out_dev, len_out, stream));
}

inline void lwe_modulus_switch_dev(int device, const uint32_t *lwe_dev, size_t len_lwe, size_t lwe_dimension, uint32_t log_n,
                                   uint32_t *exps_dev, size_t len_exps, uint32_t *neg_b_dev, size_t len_neg_b,
                                   void *stream = nullptr) {
    check(pfhe_tfhe32_modswitch_dev(device, lwe_dev, len_lwe, lwe_dimension, log_n, exps_dev, len_exps, neg_b_dev, len_neg_b,
                                  stream));
}
inline void lwe_modulus_switch_strided_dev(int device, const uint32_t *lwe_dev, size_t len_lwe, size_t lwe_dimension,
                                           uint32_t log_n, uint32_t log_stride, uint32_t *exps_dev, size_t len_exps,
                                           uint32_t *neg_b_dev, size_t len_neg_b, void *stream = nullptr) {
    check(pfhe_tfhe32_modswitch_stride_dev(device, lwe_dev, len_lwe, lwe_dimension, log_n, log_stride, exps_dev, len_exps,
                                           neg_b_dev, len_neg_b, stream));
}
inline void glwe_sample_extract(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint32_t *glwe, size_t len_glwe,
                                size_t index, uint32_t *lwe, size_t len_lwe) {
    check(pfhe_tfhe32_sample_extract(fft.handle(), glwe_dimension, glwe, len_glwe, index, lwe, len_lwe));
}
inline void glwe_sample_extract_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint32_t *glwe_dev,
                                    size_t len_glwe, size_t index, uint32_t *lwe_dev, size_t len_lwe, void *stream = nullptr) {
    check(pfhe_tfhe32_sample_extract_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, index, lwe_dev, len_lwe, stream));
}
inline void lwe_keyswitch(int device, const uint32_t *lwe_in, size_t len_in, size_t in_dimension, const uint32_t *ksk, size_t len_ksk,
                          size_t out_dimension, uint32_t log_basis, size_t decompose_length, uint32_t *lwe_out, size_t len_out) {
    check(pfhe_tfhe32_keyswitch(device, lwe_in, len_in, in_dimension, ksk, len_ksk, out_dimension, log_basis, decompose_length,
                              lwe_out, len_out));
}
inline void lwe_keyswitch_dev(int device, const uint32_t *lwe_in_dev, size_t len_in, size_t in_dimension, const uint32_t *ksk_dev,
                              size_t len_ksk, size_t out_dimension, uint32_t log_basis, size_t decompose_length,
                              uint32_t *lwe_out_dev, size_t len_out, void *stream = nullptr) {
    check(pfhe_tfhe32_keyswitch_dev(device, lwe_in_dev, len_in, in_dimension, ksk_dev, len_ksk, out_dimension, log_basis,
                                  decompose_length, lwe_out_dev, len_out, stream));
}

// The batched programmable bootstrap (pfhe_tfhe_bootstrap_*): modulus switch, ACC = X^{-b~} * TV, the blind rotation over
// lwe_dimension steps, sample extraction at index 0 and, with a key switch, the switch back to lwe_dimension.  Owns a
// blind-rotation handle and every buffer between the stages; one holder at a time.  TfheBootstrap32: the u32 torus.
class TfheBootstrap {
  public:
    TfheBootstrap(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                    size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length, bool with_keyswitch = true,
                    size_t chunk = 0, size_t grouping_factor = 1, uint32_t log_luts = 0) {
        // grouping_factor 1: the classic rotation; above 1 the multi-bit one, on (lwe_dimension / g) * 2^g keys.  log_luts
        // above 0: the many-LUT bootstrap, 2^log_luts outputs per input (output (e, i) at e * 2^log_luts + i)
        check(log_luts != 0
                  ? pfhe_tfhe_bootstrap_create_many_lut(fft.handle(), glwe_dimension, log_basis, decompose_length,
                                                        lwe_dimension, ks_log_basis, ks_decompose_length,
                                                        with_keyswitch ? 1 : 0, grouping_factor, log_luts, chunk, &h_)
              : grouping_factor == 1
                  ? pfhe_tfhe_bootstrap_create(fft.handle(), glwe_dimension, log_basis, decompose_length, lwe_dimension,
                                               ks_log_basis, ks_decompose_length, with_keyswitch ? 1 : 0, chunk, &h_)
                  : pfhe_tfhe_bootstrap_create_multibit(fft.handle(), glwe_dimension, log_basis, decompose_length,
                                                        lwe_dimension, ks_log_basis, ks_decompose_length,
                                                        with_keyswitch ? 1 : 0, grouping_factor, chunk, &h_));
    }
    ~TfheBootstrap() { pfhe_tfhe_bootstrap_destroy(h_); }
    TfheBootstrap(const TfheBootstrap &) = delete;
    TfheBootstrap &operator=(const TfheBootstrap &) = delete;
    pfhe_tfhe_bootstrap_handle *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe_bootstrap_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe_bootstrap_scratch_bytes(h_); }
    void bootstrap(const uint64_t *lwe_in, size_t len_in, const double *bsk, size_t len_bsk, const uint64_t *tv, size_t len_tv,
                   const uint64_t *ksk, size_t len_ksk, uint64_t *lwe_out, size_t len_out) {
        check(pfhe_tfhe_bootstrap(h_, lwe_in, len_in, bsk, len_bsk, tv, len_tv, ksk, len_ksk, lwe_out, len_out));
    }
    void bootstrap_dev(const uint64_t *lwe_in_dev, size_t len_in, const double *bsk_dev, size_t len_bsk, const uint64_t *tv_dev,
                       size_t len_tv, const uint64_t *ksk_dev, size_t len_ksk, uint64_t *lwe_out_dev, size_t len_out,
                       void *stream = nullptr) {
        check(pfhe_tfhe_bootstrap_dev(h_, lwe_in_dev, len_in, bsk_dev, len_bsk, tv_dev, len_tv, ksk_dev, len_ksk, lwe_out_dev,
                                      len_out, stream));
    }

  private:
    pfhe_tfhe_bootstrap_handle *h_ = nullptr;
};

class TfheBootstrap32 {
  public:
    TfheBootstrap32(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                    size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length, bool with_keyswitch = true,
                    size_t chunk = 0, size_t grouping_factor = 1, uint32_t log_luts = 0) {
        // grouping_factor 1: the classic rotation; above 1 the multi-bit one, on (lwe_dimension / g) * 2^g keys.  log_luts
        // above 0: the many-LUT bootstrap, 2^log_luts outputs per input (output (e, i) at e * 2^log_luts + i)
        check(log_luts != 0
                  ? pfhe_tfhe32_bootstrap_create_many_lut(fft.handle(), glwe_dimension, log_basis, decompose_length,
                                                          lwe_dimension, ks_log_basis, ks_decompose_length,
                                                          with_keyswitch ? 1 : 0, grouping_factor, log_luts, chunk, &h_)
              : grouping_factor == 1
                  ? pfhe_tfhe32_bootstrap_create(fft.handle(), glwe_dimension, log_basis, decompose_length, lwe_dimension,
                                               ks_log_basis, ks_decompose_length, with_keyswitch ? 1 : 0, chunk, &h_)
                  : pfhe_tfhe32_bootstrap_create_multibit(fft.handle(), glwe_dimension, log_basis, decompose_length,
                                                        lwe_dimension, ks_log_basis, ks_decompose_length,
                                                        with_keyswitch ? 1 : 0, grouping_factor, chunk, &h_));
    }
    ~TfheBootstrap32() { pfhe_tfhe32_bootstrap_destroy(h_); }
    TfheBootstrap32(const TfheBootstrap32 &) = delete;
    TfheBootstrap32 &operator=(const TfheBootstrap32 &) = delete;
    pfhe_tfhe32_bootstrap_handle *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe32_bootstrap_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe32_bootstrap_scratch_bytes(h_); }
    void bootstrap(const uint32_t *lwe_in, size_t len_in, const double *bsk, size_t len_bsk, const uint32_t *tv, size_t len_tv,
                   const uint32_t *ksk, size_t len_ksk, uint32_t *lwe_out, size_t len_out) {
        check(pfhe_tfhe32_bootstrap(h_, lwe_in, len_in, bsk, len_bsk, tv, len_tv, ksk, len_ksk, lwe_out, len_out));
    }
    void bootstrap_dev(const uint32_t *lwe_in_dev, size_t len_in, const double *bsk_dev, size_t len_bsk, const uint32_t *tv_dev,
                       size_t len_tv, const uint32_t *ksk_dev, size_t len_ksk, uint32_t *lwe_out_dev, size_t len_out,
                       void *stream = nullptr) {
        check(pfhe_tfhe32_bootstrap_dev(h_, lwe_in_dev, len_in, bsk_dev, len_bsk, tv_dev, len_tv, ksk_dev, len_ksk, lwe_out_dev,
                                      len_out, stream));
    }

  private:
    pfhe_tfhe32_bootstrap_handle *h_ = nullptr;
};

// Key generation, encryption and phase (pfhe_tfhe{,32}_lwe_body_mac*, _glwe_body_mac*, _ggsw_add_gadget_dev, _bsk_generate_dev,
// _ksk_generate_dev).  No random number is drawn: the buffers arrive holding the caller's randomness (masks uniform, bodies
// noise + message).  body_mac adds <a,s> (A * z) into the body slot, or subtracts it (the phase); the gadget call adds
// m * 2^(drop_bits + l*log_basis); the two generators write the keys TfheBootstrap takes (grouping_factor 0: the classic
// layout, 1..4: the multi-bit one).  uint64_t overloads: the u64 torus; uint32_t: the u32 torus.
inline void lwe_body_mac(int device, uint64_t *lwe, size_t len_lwe, size_t dimension, const uint64_t *key, size_t len_key,
                         bool subtract) {
    check(pfhe_tfhe_lwe_body_mac(device, lwe, len_lwe, dimension, key, len_key, subtract ? 1 : 0));
}
inline void lwe_body_mac_dev(int device, uint64_t *lwe_dev, size_t len_lwe, size_t dimension, const uint64_t *key_dev,
                             size_t len_key, bool subtract, void *stream = nullptr) {
    check(pfhe_tfhe_lwe_body_mac_dev(device, lwe_dev, len_lwe, dimension, key_dev, len_key, subtract ? 1 : 0, stream));
}
inline void glwe_body_mac(const FullComplex64FftTable &fft, size_t glwe_dimension, uint64_t *glwe, size_t len_glwe,
                          const uint64_t *key, size_t len_key, bool subtract) {
    check(pfhe_tfhe_glwe_body_mac(fft.handle(), glwe_dimension, glwe, len_glwe, key, len_key, subtract ? 1 : 0));
}
inline void glwe_body_mac_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, uint64_t *glwe_dev, size_t len_glwe,
                              const uint64_t *key_dev, size_t len_key, bool subtract, void *stream = nullptr) {
    check(pfhe_tfhe_glwe_body_mac_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, key_dev, len_key, subtract ? 1 : 0,
          stream));
}
inline void ggsw_add_gadget_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis,
                                size_t decompose_length, uint64_t *ggsw_dev, size_t len_ggsw, const uint64_t *messages_dev,
                                size_t len_messages, void *stream = nullptr) {
    check(pfhe_tfhe_ggsw_add_gadget_dev(fft.handle(), glwe_dimension, log_basis, decompose_length, ggsw_dev, len_ggsw,
          messages_dev, len_messages, stream));
}
inline void tfhe_generate_bsk_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis,
                                  size_t decompose_length, size_t grouping_factor, const uint64_t *lwe_key_dev,
                                  size_t lwe_dimension, const uint64_t *glwe_key_dev, size_t len_glwe_key,
                                  uint64_t *ggsw_torus_dev, size_t len_ggsw, double *bsk_out_dev, size_t len_bsk,
                                  void *stream = nullptr) {
    check(pfhe_tfhe_bsk_generate_dev(fft.handle(), glwe_dimension, log_basis, decompose_length, grouping_factor, lwe_key_dev,
          lwe_dimension, glwe_key_dev, len_glwe_key, ggsw_torus_dev, len_ggsw, bsk_out_dev, len_bsk, stream));
}
inline void tfhe_generate_ksk_dev(int device, const uint64_t *key_in_dev, size_t in_dimension, const uint64_t *key_out_dev,
                                  size_t out_dimension, uint32_t log_basis, size_t decompose_length, uint64_t *ksk_dev,
                                  size_t len_ksk, void *stream = nullptr) {
    check(pfhe_tfhe_ksk_generate_dev(device, key_in_dev, in_dimension, key_out_dev, out_dimension, log_basis, decompose_length,
          ksk_dev, len_ksk, stream));
}

inline void lwe_body_mac(int device, uint32_t *lwe, size_t len_lwe, size_t dimension, const uint32_t *key, size_t len_key,
                         bool subtract) {
    check(pfhe_tfhe32_lwe_body_mac(device, lwe, len_lwe, dimension, key, len_key, subtract ? 1 : 0));
}
inline void lwe_body_mac_dev(int device, uint32_t *lwe_dev, size_t len_lwe, size_t dimension, const uint32_t *key_dev,
                             size_t len_key, bool subtract, void *stream = nullptr) {
    check(pfhe_tfhe32_lwe_body_mac_dev(device, lwe_dev, len_lwe, dimension, key_dev, len_key, subtract ? 1 : 0, stream));
}
inline void glwe_body_mac(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t *glwe, size_t len_glwe,
                          const uint32_t *key, size_t len_key, bool subtract) {
    check(pfhe_tfhe32_glwe_body_mac(fft.handle(), glwe_dimension, glwe, len_glwe, key, len_key, subtract ? 1 : 0));
}
inline void glwe_body_mac_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t *glwe_dev, size_t len_glwe,
                              const uint32_t *key_dev, size_t len_key, bool subtract, void *stream = nullptr) {
    check(pfhe_tfhe32_glwe_body_mac_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, key_dev, len_key, subtract ? 1 : 0,
          stream));
}
inline void ggsw_add_gadget_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis,
                                size_t decompose_length, uint32_t *ggsw_dev, size_t len_ggsw, const uint32_t *messages_dev,
                                size_t len_messages, void *stream = nullptr) {
    check(pfhe_tfhe32_ggsw_add_gadget_dev(fft.handle(), glwe_dimension, log_basis, decompose_length, ggsw_dev, len_ggsw,
          messages_dev, len_messages, stream));
}
inline void tfhe_generate_bsk_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis,
                                  size_t decompose_length, size_t grouping_factor, const uint32_t *lwe_key_dev,
                                  size_t lwe_dimension, const uint32_t *glwe_key_dev, size_t len_glwe_key,
                                  uint32_t *ggsw_torus_dev, size_t len_ggsw, double *bsk_out_dev, size_t len_bsk,
                                  void *stream = nullptr) {
    check(pfhe_tfhe32_bsk_generate_dev(fft.handle(), glwe_dimension, log_basis, decompose_length, grouping_factor, lwe_key_dev,
          lwe_dimension, glwe_key_dev, len_glwe_key, ggsw_torus_dev, len_ggsw, bsk_out_dev, len_bsk, stream));
}
inline void tfhe_generate_ksk_dev(int device, const uint32_t *key_in_dev, size_t in_dimension, const uint32_t *key_out_dev,
                                  size_t out_dimension, uint32_t log_basis, size_t decompose_length, uint32_t *ksk_dev,
                                  size_t len_ksk, void *stream = nullptr) {
    check(pfhe_tfhe32_ksk_generate_dev(device, key_in_dev, in_dimension, key_out_dev, out_dimension, log_basis, decompose_length,
          ksk_dev, len_ksk, stream));
}

// Packing (pfhe_tfhe{,32}_pack_keyswitch*, _pksk_generate_dev, _sample_extract_first_few*, _multimsg_extract*): `count` LWE
// ciphertexts per group into one GLWE under the packing key (in_dimension x ell GLWE rows, generated in place from the
// caller's randomness), Rlwe::extract_first_few_lwe per mask polynomial (the MultiMsgLwe layout) and its expansion into
// `count` LWE ciphertexts (MultiMsgLwe::extract_rlwe_mode at every index).  uint64_t overloads: the u64 torus; uint32_t: u32.
inline void lwe_pack_keyswitch(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint64_t *lwe_in, size_t len_in,
                               size_t in_dimension, size_t count, const uint64_t *pksk, size_t len_pksk, uint32_t log_basis,
                               size_t decompose_length, uint64_t *glwe_out, size_t len_out) {
    check(pfhe_tfhe_pack_keyswitch(fft.handle(), glwe_dimension, lwe_in, len_in, in_dimension, count, pksk, len_pksk, log_basis,
          decompose_length, glwe_out, len_out));
}
inline void lwe_pack_keyswitch_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint64_t *lwe_in_dev, size_t len_in,
                                   size_t in_dimension, size_t count, const uint64_t *pksk_dev, size_t len_pksk,
                                   uint32_t log_basis, size_t decompose_length, uint64_t *glwe_out_dev, size_t len_out,
                                   void *stream = nullptr) {
    check(pfhe_tfhe_pack_keyswitch_dev(fft.handle(), glwe_dimension, lwe_in_dev, len_in, in_dimension, count, pksk_dev, len_pksk,
          log_basis, decompose_length, glwe_out_dev, len_out, stream));
}
inline void tfhe_generate_pksk_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint64_t *key_in_dev,
                                   size_t in_dimension, const uint64_t *glwe_key_dev, size_t len_glwe_key, uint32_t log_basis,
                                   size_t decompose_length, uint64_t *pksk_dev, size_t len_pksk, void *stream = nullptr) {
    check(pfhe_tfhe_pksk_generate_dev(fft.handle(), glwe_dimension, key_in_dev, in_dimension, glwe_key_dev, len_glwe_key,
          log_basis, decompose_length, pksk_dev, len_pksk, stream));
}
inline void glwe_sample_extract_first_few(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint64_t *glwe,
                                          size_t len_glwe, size_t count, uint64_t *multi, size_t len_multi) {
    check(pfhe_tfhe_sample_extract_first_few(fft.handle(), glwe_dimension, glwe, len_glwe, count, multi, len_multi));
}
inline void glwe_sample_extract_first_few_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint64_t *glwe_dev,
                                              size_t len_glwe, size_t count, uint64_t *multi_dev, size_t len_multi,
                                              void *stream = nullptr) {
    check(pfhe_tfhe_sample_extract_first_few_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, count, multi_dev, len_multi,
          stream));
}
inline void multimsg_lwe_extract(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint64_t *multi, size_t len_multi,
                                 size_t count, uint64_t *lwe, size_t len_lwe) {
    check(pfhe_tfhe_multimsg_extract(fft.handle(), glwe_dimension, multi, len_multi, count, lwe, len_lwe));
}
inline void multimsg_lwe_extract_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint64_t *multi_dev,
                                     size_t len_multi, size_t count, uint64_t *lwe_dev, size_t len_lwe, void *stream = nullptr) {
    check(pfhe_tfhe_multimsg_extract_dev(fft.handle(), glwe_dimension, multi_dev, len_multi, count, lwe_dev, len_lwe, stream));
}

inline void lwe_pack_keyswitch(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint32_t *lwe_in, size_t len_in,
                               size_t in_dimension, size_t count, const uint32_t *pksk, size_t len_pksk, uint32_t log_basis,
                               size_t decompose_length, uint32_t *glwe_out, size_t len_out) {
    check(pfhe_tfhe32_pack_keyswitch(fft.handle(), glwe_dimension, lwe_in, len_in, in_dimension, count, pksk, len_pksk, log_basis,
          decompose_length, glwe_out, len_out));
}
inline void lwe_pack_keyswitch_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint32_t *lwe_in_dev, size_t len_in,
                                   size_t in_dimension, size_t count, const uint32_t *pksk_dev, size_t len_pksk,
                                   uint32_t log_basis, size_t decompose_length, uint32_t *glwe_out_dev, size_t len_out,
                                   void *stream = nullptr) {
    check(pfhe_tfhe32_pack_keyswitch_dev(fft.handle(), glwe_dimension, lwe_in_dev, len_in, in_dimension, count, pksk_dev, len_pksk,
          log_basis, decompose_length, glwe_out_dev, len_out, stream));
}
inline void tfhe_generate_pksk_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint32_t *key_in_dev,
                                   size_t in_dimension, const uint32_t *glwe_key_dev, size_t len_glwe_key, uint32_t log_basis,
                                   size_t decompose_length, uint32_t *pksk_dev, size_t len_pksk, void *stream = nullptr) {
    check(pfhe_tfhe32_pksk_generate_dev(fft.handle(), glwe_dimension, key_in_dev, in_dimension, glwe_key_dev, len_glwe_key,
          log_basis, decompose_length, pksk_dev, len_pksk, stream));
}
inline void glwe_sample_extract_first_few(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint32_t *glwe,
                                          size_t len_glwe, size_t count, uint32_t *multi, size_t len_multi) {
    check(pfhe_tfhe32_sample_extract_first_few(fft.handle(), glwe_dimension, glwe, len_glwe, count, multi, len_multi));
}
inline void glwe_sample_extract_first_few_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint32_t *glwe_dev,
                                              size_t len_glwe, size_t count, uint32_t *multi_dev, size_t len_multi,
                                              void *stream = nullptr) {
    check(pfhe_tfhe32_sample_extract_first_few_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, count, multi_dev, len_multi,
          stream));
}
inline void multimsg_lwe_extract(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint32_t *multi, size_t len_multi,
                                 size_t count, uint32_t *lwe, size_t len_lwe) {
    check(pfhe_tfhe32_multimsg_extract(fft.handle(), glwe_dimension, multi, len_multi, count, lwe, len_lwe));
}
inline void multimsg_lwe_extract_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint32_t *multi_dev,
                                     size_t len_multi, size_t count, uint32_t *lwe_dev, size_t len_lwe, void *stream = nullptr) {
    check(pfhe_tfhe32_multimsg_extract_dev(fft.handle(), glwe_dimension, multi_dev, len_multi, count, lwe_dev, len_lwe, stream));
}

// The packing key switch in the Fourier domain (pfhe_tfhe{,32}_packfft_*, _pack_keyswitch_fft*): lwe_pack_keyswitch's rule
// as one external product of in_dimension * ell rows against the half-spectrum key of tfhe_pack_key_fourier_dev.  Approximate
// as the TFHE product is and opt-in: 1 <= log N <= 11, 1 <= glwe_dimension <= 3; the exact call above serves every shape.
// The context owns the partial sums of `chunk` groups; one holder at a time.
class TfhePackFftContext {
  public:
    TfhePackFftContext(const FullComplex64FftTable &fft, size_t glwe_dimension, size_t in_dimension, uint32_t log_basis,
                       size_t decompose_length = 0, size_t chunk = 0) {
        check(pfhe_tfhe_packfft_plan_create(fft.handle(), glwe_dimension, in_dimension, log_basis, decompose_length, chunk, &h_));
    }
    ~TfhePackFftContext() { pfhe_tfhe_packfft_plan_destroy(h_); }
    TfhePackFftContext(const TfhePackFftContext &) = delete;
    TfhePackFftContext &operator=(const TfhePackFftContext &) = delete;
    pfhe_tfhe_packfft_plan *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe_packfft_plan_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe_packfft_plan_scratch_bytes(h_); }

  private:
    pfhe_tfhe_packfft_plan *h_ = nullptr;
};

// the u32 torus
class TfhePackFftContext32 {
  public:
    TfhePackFftContext32(const FullComplex64FftTable &fft, size_t glwe_dimension, size_t in_dimension, uint32_t log_basis,
                         size_t decompose_length = 0, size_t chunk = 0) {
        check(pfhe_tfhe32_packfft_plan_create(fft.handle(), glwe_dimension, in_dimension, log_basis, decompose_length, chunk, &h_));
    }
    ~TfhePackFftContext32() { pfhe_tfhe32_packfft_plan_destroy(h_); }
    TfhePackFftContext32(const TfhePackFftContext32 &) = delete;
    TfhePackFftContext32 &operator=(const TfhePackFftContext32 &) = delete;
    pfhe_tfhe32_packfft_plan *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe32_packfft_plan_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe32_packfft_plan_scratch_bytes(h_); }

  private:
    pfhe_tfhe32_packfft_plan *h_ = nullptr;
};

inline void tfhe_pack_key_fourier_dev(const uint64_t *pksk_dev, size_t len_pksk, double *fkey_dev, size_t len_fkey,
                                      TfhePackFftContext &context, void *stream = nullptr) {
    check(pfhe_tfhe_packfft_key_dev(context.handle(), pksk_dev, len_pksk, fkey_dev, len_fkey, stream));
}
inline void lwe_pack_keyswitch_fft(const uint64_t *lwe_in, size_t len_in, size_t count, const double *fkey, size_t len_fkey,
                                   uint64_t *glwe_out, size_t len_out, TfhePackFftContext &context) {
    check(pfhe_tfhe_pack_keyswitch_fft(context.handle(), lwe_in, len_in, count, fkey, len_fkey, glwe_out, len_out));
}
inline void lwe_pack_keyswitch_fft_dev(const uint64_t *lwe_in_dev, size_t len_in, size_t count, const double *fkey_dev,
                                       size_t len_fkey, uint64_t *glwe_out_dev, size_t len_out, TfhePackFftContext &context,
                                       void *stream = nullptr) {
    check(pfhe_tfhe_pack_keyswitch_fft_dev(context.handle(), lwe_in_dev, len_in, count, fkey_dev, len_fkey, glwe_out_dev, len_out,
          stream));
}
inline void tfhe_pack_key_fourier_dev(const uint32_t *pksk_dev, size_t len_pksk, double *fkey_dev, size_t len_fkey,
                                      TfhePackFftContext32 &context, void *stream = nullptr) {
    check(pfhe_tfhe32_packfft_key_dev(context.handle(), pksk_dev, len_pksk, fkey_dev, len_fkey, stream));
}
inline void lwe_pack_keyswitch_fft(const uint32_t *lwe_in, size_t len_in, size_t count, const double *fkey, size_t len_fkey,
                                   uint32_t *glwe_out, size_t len_out, TfhePackFftContext32 &context) {
    check(pfhe_tfhe32_pack_keyswitch_fft(context.handle(), lwe_in, len_in, count, fkey, len_fkey, glwe_out, len_out));
}
inline void lwe_pack_keyswitch_fft_dev(const uint32_t *lwe_in_dev, size_t len_in, size_t count, const double *fkey_dev,
                                       size_t len_fkey, uint32_t *glwe_out_dev, size_t len_out, TfhePackFftContext32 &context,
                                       void *stream = nullptr) {
    check(pfhe_tfhe32_pack_keyswitch_fft_dev(context.handle(), lwe_in_dev, len_in, count, fkey_dev, len_fkey, glwe_out_dev, len_out,
          stream));
}

// The circuit bootstrap (pfhe_tfhe{,32}_private_keyswitch*, _pfksk_generate_dev, _cbs_*): the private functional key switch
// turns batch x levels LWE ciphertexts into GGSW-shaped blocks whose row (u, l) has the phase f_u of input (e, l), under the
// key tfhe_generate_pfksk_dev writes in place from the caller's randomness; TfheCircuitBootstrap runs, per input bit and
// level of the output basis, modulus switch, ACC = X^{-b~} * (-g_l/2), the blind rotation, extraction with g_l/2 added and
// that key switch, and gives a torus-form GGSW of the bit.  uint64_t overloads: the u64 torus; uint32_t: u32.
inline void lwe_private_keyswitch(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint64_t *lwe_in, size_t len_in,
                                  size_t in_dimension, size_t levels, const uint64_t *pfksk, size_t len_pfksk,
                                  uint32_t log_basis, size_t decompose_length, uint64_t *out, size_t len_out) {
    check(pfhe_tfhe_private_keyswitch(fft.handle(), glwe_dimension, lwe_in, len_in, in_dimension, levels, pfksk, len_pfksk,
          log_basis, decompose_length, out, len_out));
}
inline void lwe_private_keyswitch_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint64_t *lwe_in_dev,
                                      size_t len_in, size_t in_dimension, size_t levels, const uint64_t *pfksk_dev,
                                      size_t len_pfksk, uint32_t log_basis, size_t decompose_length, uint64_t *out_dev,
                                      size_t len_out, void *stream = nullptr) {
    check(pfhe_tfhe_private_keyswitch_dev(fft.handle(), glwe_dimension, lwe_in_dev, len_in, in_dimension, levels, pfksk_dev,
          len_pfksk, log_basis, decompose_length, out_dev, len_out, stream));
}
inline void tfhe_generate_pfksk_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint64_t *key_in_dev,
                                    size_t in_dimension, const uint64_t *glwe_key_dev, size_t len_glwe_key, uint32_t log_basis,
                                    size_t decompose_length, uint64_t *pfksk_dev, size_t len_pfksk, void *stream = nullptr) {
    check(pfhe_tfhe_pfksk_generate_dev(fft.handle(), glwe_dimension, key_in_dev, in_dimension, glwe_key_dev, len_glwe_key,
          log_basis, decompose_length, pfksk_dev, len_pfksk, stream));
}

inline void lwe_private_keyswitch(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint32_t *lwe_in, size_t len_in,
                                  size_t in_dimension, size_t levels, const uint32_t *pfksk, size_t len_pfksk,
                                  uint32_t log_basis, size_t decompose_length, uint32_t *out, size_t len_out) {
    check(pfhe_tfhe32_private_keyswitch(fft.handle(), glwe_dimension, lwe_in, len_in, in_dimension, levels, pfksk, len_pfksk,
          log_basis, decompose_length, out, len_out));
}
inline void lwe_private_keyswitch_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint32_t *lwe_in_dev,
                                      size_t len_in, size_t in_dimension, size_t levels, const uint32_t *pfksk_dev,
                                      size_t len_pfksk, uint32_t log_basis, size_t decompose_length, uint32_t *out_dev,
                                      size_t len_out, void *stream = nullptr) {
    check(pfhe_tfhe32_private_keyswitch_dev(fft.handle(), glwe_dimension, lwe_in_dev, len_in, in_dimension, levels, pfksk_dev,
          len_pfksk, log_basis, decompose_length, out_dev, len_out, stream));
}
inline void tfhe_generate_pfksk_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const uint32_t *key_in_dev,
                                    size_t in_dimension, const uint32_t *glwe_key_dev, size_t len_glwe_key, uint32_t log_basis,
                                    size_t decompose_length, uint32_t *pfksk_dev, size_t len_pfksk, void *stream = nullptr) {
    check(pfhe_tfhe32_pfksk_generate_dev(fft.handle(), glwe_dimension, key_in_dev, in_dimension, glwe_key_dev, len_glwe_key,
          log_basis, decompose_length, pfksk_dev, len_pfksk, stream));
}

// Owns a blind-rotation handle and every buffer between the stages for `chunk` inputs; one holder at a time.
// TfheCircuitBootstrap32: the u32 torus.
class TfheCircuitBootstrap {
  public:
    TfheCircuitBootstrap(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
        size_t lwe_dimension, uint32_t cbs_log_basis, size_t cbs_decompose_length, uint32_t pfks_log_basis,
        size_t pfks_decompose_length, size_t chunk = 0) {
        check(pfhe_tfhe_cbs_create(fft.handle(), glwe_dimension, log_basis, decompose_length, lwe_dimension, cbs_log_basis,
                                   cbs_decompose_length, pfks_log_basis, pfks_decompose_length, chunk, &h_));
    }
    // with options (pfhe_tfhe_cbs_create_with): grouping_factor above 1 runs the multi-bit rotation on its key;
    // shared_rotation runs one rotation per input for all levels of the output basis (many-LUT)
    TfheCircuitBootstrap(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
        size_t lwe_dimension, uint32_t cbs_log_basis, size_t cbs_decompose_length, uint32_t pfks_log_basis,
        size_t pfks_decompose_length, size_t chunk, size_t grouping_factor, bool shared_rotation) {
        check(pfhe_tfhe_cbs_create_with(fft.handle(), glwe_dimension, log_basis, decompose_length, lwe_dimension, cbs_log_basis,
                                        cbs_decompose_length, pfks_log_basis, pfks_decompose_length, grouping_factor,
                                        shared_rotation ? 1 : 0, chunk, &h_));
    }
    ~TfheCircuitBootstrap() { pfhe_tfhe_cbs_destroy(h_); }
    TfheCircuitBootstrap(const TfheCircuitBootstrap &) = delete;
    TfheCircuitBootstrap &operator=(const TfheCircuitBootstrap &) = delete;
    pfhe_tfhe_cbs_handle *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe_cbs_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe_cbs_scratch_bytes(h_); }
    void circuit_bootstrap(const uint64_t *lwe_in, size_t len_in, const double *bsk, size_t len_bsk, const uint64_t *pfksk,
                           size_t len_pfksk, uint64_t *ggsw_out, size_t len_out) {
        check(pfhe_tfhe_cbs(h_, lwe_in, len_in, bsk, len_bsk, pfksk, len_pfksk, ggsw_out, len_out));
    }
    void circuit_bootstrap_dev(const uint64_t *lwe_in_dev, size_t len_in, const double *bsk_dev, size_t len_bsk,
                               const uint64_t *pfksk_dev, size_t len_pfksk, uint64_t *ggsw_out_dev, size_t len_out,
                               void *stream = nullptr) {
        check(pfhe_tfhe_cbs_dev(h_, lwe_in_dev, len_in, bsk_dev, len_bsk, pfksk_dev, len_pfksk, ggsw_out_dev, len_out, stream));
    }

  private:
    pfhe_tfhe_cbs_handle *h_ = nullptr;
};

class TfheCircuitBootstrap32 {
  public:
    TfheCircuitBootstrap32(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
        size_t lwe_dimension, uint32_t cbs_log_basis, size_t cbs_decompose_length, uint32_t pfks_log_basis,
        size_t pfks_decompose_length, size_t chunk = 0) {
        check(pfhe_tfhe32_cbs_create(fft.handle(), glwe_dimension, log_basis, decompose_length, lwe_dimension, cbs_log_basis,
                                   cbs_decompose_length, pfks_log_basis, pfks_decompose_length, chunk, &h_));
    }
    TfheCircuitBootstrap32(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
        size_t lwe_dimension, uint32_t cbs_log_basis, size_t cbs_decompose_length, uint32_t pfks_log_basis,
        size_t pfks_decompose_length, size_t chunk, size_t grouping_factor, bool shared_rotation) {
        check(pfhe_tfhe32_cbs_create_with(fft.handle(), glwe_dimension, log_basis, decompose_length, lwe_dimension,
                                          cbs_log_basis, cbs_decompose_length, pfks_log_basis, pfks_decompose_length,
                                          grouping_factor, shared_rotation ? 1 : 0, chunk, &h_));
    }
    ~TfheCircuitBootstrap32() { pfhe_tfhe32_cbs_destroy(h_); }
    TfheCircuitBootstrap32(const TfheCircuitBootstrap32 &) = delete;
    TfheCircuitBootstrap32 &operator=(const TfheCircuitBootstrap32 &) = delete;
    pfhe_tfhe32_cbs_handle *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe32_cbs_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe32_cbs_scratch_bytes(h_); }
    void circuit_bootstrap(const uint32_t *lwe_in, size_t len_in, const double *bsk, size_t len_bsk, const uint32_t *pfksk,
                           size_t len_pfksk, uint32_t *ggsw_out, size_t len_out) {
        check(pfhe_tfhe32_cbs(h_, lwe_in, len_in, bsk, len_bsk, pfksk, len_pfksk, ggsw_out, len_out));
    }
    void circuit_bootstrap_dev(const uint32_t *lwe_in_dev, size_t len_in, const double *bsk_dev, size_t len_bsk,
                               const uint32_t *pfksk_dev, size_t len_pfksk, uint32_t *ggsw_out_dev, size_t len_out,
                               void *stream = nullptr) {
        check(pfhe_tfhe32_cbs_dev(h_, lwe_in_dev, len_in, bsk_dev, len_bsk, pfksk_dev, len_pfksk, ggsw_out_dev, len_out, stream));
    }

  private:
    pfhe_tfhe32_cbs_handle *h_ = nullptr;
};

// The batched CMUX with a Fourier GGSW selector per group of per_key ciphertexts (out[i] = d0[i] +
// external_product_to(d1[i] - d0[i], keys[i / per_key]); out may be d0 or d1) and the tree that selects one of 2^depth GLWE
// ciphertexts by depth selectors per input (pfhe_tfhe{,32}_cmux_tree_*, _cmux, _cmux_dev).  Owns the node buffers of `chunk`
// inputs and, off the fused shape, a product plan; one holder at a time.  TfheCmuxTree32: the u32 torus.
class TfheCmuxTree {
  public:
    TfheCmuxTree(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                 size_t depth, size_t chunk = 0) {
        check(pfhe_tfhe_cmux_tree_create(fft.handle(), glwe_dimension, log_basis, decompose_length, depth, chunk, &h_));
    }
    ~TfheCmuxTree() { pfhe_tfhe_cmux_tree_destroy(h_); }
    TfheCmuxTree(const TfheCmuxTree &) = delete;
    TfheCmuxTree &operator=(const TfheCmuxTree &) = delete;
    pfhe_tfhe_cmux_tree_handle *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe_cmux_tree_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe_cmux_tree_scratch_bytes(h_); }
    void cmux(const uint64_t *d0, size_t len_d0, const uint64_t *d1, size_t len_d1, const double *keys, size_t len_keys,
              size_t per_key, uint64_t *out, size_t len_out) {
        check(pfhe_tfhe_cmux(h_, d0, len_d0, d1, len_d1, keys, len_keys, per_key, out, len_out));
    }
    void cmux_dev(const uint64_t *d0_dev, size_t len_d0, const uint64_t *d1_dev, size_t len_d1, const double *keys_dev,
                  size_t len_keys, size_t per_key, uint64_t *out_dev, size_t len_out, void *stream = nullptr) {
        check(pfhe_tfhe_cmux_dev(h_, d0_dev, len_d0, d1_dev, len_d1, keys_dev, len_keys, per_key, out_dev, len_out, stream));
    }
    void cmux_tree(const uint64_t *table, size_t len_table, const double *selectors, size_t len_selectors, uint64_t *out,
                   size_t len_out) {
        check(pfhe_tfhe_cmux_tree(h_, table, len_table, selectors, len_selectors, out, len_out));
    }
    void cmux_tree_dev(const uint64_t *table_dev, size_t len_table, const double *selectors_dev, size_t len_selectors,
                       uint64_t *out_dev, size_t len_out, void *stream = nullptr) {
        check(pfhe_tfhe_cmux_tree_dev(h_, table_dev, len_table, selectors_dev, len_selectors, out_dev, len_out, stream));
    }

  private:
    pfhe_tfhe_cmux_tree_handle *h_ = nullptr;
};

class TfheCmuxTree32 {
  public:
    TfheCmuxTree32(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                   size_t depth, size_t chunk = 0) {
        check(pfhe_tfhe32_cmux_tree_create(fft.handle(), glwe_dimension, log_basis, decompose_length, depth, chunk, &h_));
    }
    ~TfheCmuxTree32() { pfhe_tfhe32_cmux_tree_destroy(h_); }
    TfheCmuxTree32(const TfheCmuxTree32 &) = delete;
    TfheCmuxTree32 &operator=(const TfheCmuxTree32 &) = delete;
    pfhe_tfhe32_cmux_tree_handle *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe32_cmux_tree_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe32_cmux_tree_scratch_bytes(h_); }
    void cmux(const uint32_t *d0, size_t len_d0, const uint32_t *d1, size_t len_d1, const double *keys, size_t len_keys,
              size_t per_key, uint32_t *out, size_t len_out) {
        check(pfhe_tfhe32_cmux(h_, d0, len_d0, d1, len_d1, keys, len_keys, per_key, out, len_out));
    }
    void cmux_dev(const uint32_t *d0_dev, size_t len_d0, const uint32_t *d1_dev, size_t len_d1, const double *keys_dev,
                  size_t len_keys, size_t per_key, uint32_t *out_dev, size_t len_out, void *stream = nullptr) {
        check(pfhe_tfhe32_cmux_dev(h_, d0_dev, len_d0, d1_dev, len_d1, keys_dev, len_keys, per_key, out_dev, len_out, stream));
    }
    void cmux_tree(const uint32_t *table, size_t len_table, const double *selectors, size_t len_selectors, uint32_t *out,
                   size_t len_out) {
        check(pfhe_tfhe32_cmux_tree(h_, table, len_table, selectors, len_selectors, out, len_out));
    }
    void cmux_tree_dev(const uint32_t *table_dev, size_t len_table, const double *selectors_dev, size_t len_selectors,
                       uint32_t *out_dev, size_t len_out, void *stream = nullptr) {
        check(pfhe_tfhe32_cmux_tree_dev(h_, table_dev, len_table, selectors_dev, len_selectors, out_dev, len_out, stream));
    }

  private:
    pfhe_tfhe32_cmux_tree_handle *h_ = nullptr;
};

// The GLWE automorphism X -> X^t with its key switch (out = (0, .., 0, sigma_t(B)) - sum_j sum_l d_l(sigma_t(A_j)) key[j][l],
// key the k*ell mask rows of a Fourier GGSW; t = 1 is a plain key switch; out may not overlap in) and the homomorphic trace
// of `steps` steps built from it (ACC += automorphism(ACC, keys[s-1], 2^(log N - s + 1) + 1); out may be in; the factor
// 2^steps stays in the result) (pfhe_tfhe{,32}_glwe_trace_*, _glwe_automorphism*).  Owns, off the fused shape, the buffers
// of `chunk` ciphertexts; one holder at a time.  The keys come from pfhe_tfhe*_gksk_generate_dev, the embedding of an LWE
// ciphertext from pfhe_tfhe*_lwe_embed*, both stateless.  TfheGlweTrace32: the u32 torus.
class TfheGlweTrace {
  public:
    TfheGlweTrace(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                  size_t chunk = 0) {
        check(pfhe_tfhe_glwe_trace_create(fft.handle(), glwe_dimension, log_basis, decompose_length, chunk, &h_));
    }
    ~TfheGlweTrace() { pfhe_tfhe_glwe_trace_destroy(h_); }
    TfheGlweTrace(const TfheGlweTrace &) = delete;
    TfheGlweTrace &operator=(const TfheGlweTrace &) = delete;
    pfhe_tfhe_glwe_trace_handle *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe_glwe_trace_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe_glwe_trace_scratch_bytes(h_); }
    void automorphism(const uint64_t *in, size_t len_in, const double *key, size_t len_key, uint32_t t, uint64_t *out,
                      size_t len_out) {
        check(pfhe_tfhe_glwe_automorphism(h_, in, len_in, key, len_key, t, out, len_out));
    }
    void automorphism_dev(const uint64_t *in_dev, size_t len_in, const double *key_dev, size_t len_key, uint32_t t,
                          uint64_t *out_dev, size_t len_out, void *stream = nullptr) {
        check(pfhe_tfhe_glwe_automorphism_dev(h_, in_dev, len_in, key_dev, len_key, t, out_dev, len_out, stream));
    }
    void trace(const uint64_t *in, size_t len_in, const double *keys, size_t len_keys, size_t steps, uint64_t *out,
               size_t len_out) {
        check(pfhe_tfhe_glwe_trace(h_, in, len_in, keys, len_keys, steps, out, len_out));
    }
    void trace_dev(const uint64_t *in_dev, size_t len_in, const double *keys_dev, size_t len_keys, size_t steps,
                   uint64_t *out_dev, size_t len_out, void *stream = nullptr) {
        check(pfhe_tfhe_glwe_trace_dev(h_, in_dev, len_in, keys_dev, len_keys, steps, out_dev, len_out, stream));
    }

  private:
    pfhe_tfhe_glwe_trace_handle *h_ = nullptr;
};

class TfheGlweTrace32 {
  public:
    TfheGlweTrace32(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                    size_t chunk = 0) {
        check(pfhe_tfhe32_glwe_trace_create(fft.handle(), glwe_dimension, log_basis, decompose_length, chunk, &h_));
    }
    ~TfheGlweTrace32() { pfhe_tfhe32_glwe_trace_destroy(h_); }
    TfheGlweTrace32(const TfheGlweTrace32 &) = delete;
    TfheGlweTrace32 &operator=(const TfheGlweTrace32 &) = delete;
    pfhe_tfhe32_glwe_trace_handle *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe32_glwe_trace_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe32_glwe_trace_scratch_bytes(h_); }
    void automorphism(const uint32_t *in, size_t len_in, const double *key, size_t len_key, uint32_t t, uint32_t *out,
                      size_t len_out) {
        check(pfhe_tfhe32_glwe_automorphism(h_, in, len_in, key, len_key, t, out, len_out));
    }
    void automorphism_dev(const uint32_t *in_dev, size_t len_in, const double *key_dev, size_t len_key, uint32_t t,
                          uint32_t *out_dev, size_t len_out, void *stream = nullptr) {
        check(pfhe_tfhe32_glwe_automorphism_dev(h_, in_dev, len_in, key_dev, len_key, t, out_dev, len_out, stream));
    }
    void trace(const uint32_t *in, size_t len_in, const double *keys, size_t len_keys, size_t steps, uint32_t *out,
               size_t len_out) {
        check(pfhe_tfhe32_glwe_trace(h_, in, len_in, keys, len_keys, steps, out, len_out));
    }
    void trace_dev(const uint32_t *in_dev, size_t len_in, const double *keys_dev, size_t len_keys, size_t steps,
                   uint32_t *out_dev, size_t len_out, void *stream = nullptr) {
        check(pfhe_tfhe32_glwe_trace_dev(h_, in_dev, len_in, keys_dev, len_keys, steps, out_dev, len_out, stream));
    }

  private:
    pfhe_tfhe32_glwe_trace_handle *h_ = nullptr;
};

// A look-up table of 2^(tree_depth + rot_bits) entries on encrypted bits: a CMUX tree over the high bits, the rotation by
// the low bits (acc += external_product_to(X^{2N - 2^(j+log_stride)} acc - acc, the input's key of bit j); out may be inp)
// and sample extraction at the indices below `extract` (pfhe_tfhe{,32}_lut_*, _rotate_by_bits*, _lut_eval*).  Owns the
// buffers of `chunk` inputs of `outputs` look-ups each; one holder at a time.  TfheLut32: the u32 torus.
class TfheLut {
  public:
    TfheLut(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
            size_t tree_depth, size_t rot_bits, size_t outputs = 1, size_t log_stride = 0, size_t chunk = 0) {
        check(pfhe_tfhe_lut_create(fft.handle(), glwe_dimension, log_basis, decompose_length, tree_depth, rot_bits, log_stride,
                                    outputs, chunk, &h_));
    }
    ~TfheLut() { pfhe_tfhe_lut_destroy(h_); }
    TfheLut(const TfheLut &) = delete;
    TfheLut &operator=(const TfheLut &) = delete;
    pfhe_tfhe_lut_handle *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe_lut_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe_lut_scratch_bytes(h_); }
    void rotate_by_bits(const uint64_t *inp, size_t len_inp, const double *keys, size_t len_keys, size_t keys_per_input,
                        size_t first_key, uint64_t *out, size_t len_out) {
        check(pfhe_tfhe_rotate_by_bits(h_, inp, len_inp, keys, len_keys, keys_per_input, first_key, out, len_out));
    }
    void rotate_by_bits_dev(const uint64_t *inp_dev, size_t len_inp, const double *keys_dev, size_t len_keys,
                            size_t keys_per_input, size_t first_key, uint64_t *out_dev, size_t len_out, void *stream = nullptr) {
        check(pfhe_tfhe_rotate_by_bits_dev(h_, inp_dev, len_inp, keys_dev, len_keys, keys_per_input, first_key, out_dev, len_out,
                                            stream));
    }
    void lut_eval(const uint64_t *table, size_t len_table, const double *selectors, size_t len_selectors, size_t extract,
                  uint64_t *out, size_t len_out) {
        check(pfhe_tfhe_lut_eval(h_, table, len_table, selectors, len_selectors, extract, out, len_out));
    }
    void lut_eval_dev(const uint64_t *table_dev, size_t len_table, const double *selectors_dev, size_t len_selectors,
                      size_t extract, uint64_t *out_dev, size_t len_out, void *stream = nullptr) {
        check(pfhe_tfhe_lut_eval_dev(h_, table_dev, len_table, selectors_dev, len_selectors, extract, out_dev, len_out, stream));
    }

  private:
    pfhe_tfhe_lut_handle *h_ = nullptr;
};

class TfheLut32 {
  public:
    TfheLut32(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
              size_t tree_depth, size_t rot_bits, size_t outputs = 1, size_t log_stride = 0, size_t chunk = 0) {
        check(pfhe_tfhe32_lut_create(fft.handle(), glwe_dimension, log_basis, decompose_length, tree_depth, rot_bits, log_stride,
                                      outputs, chunk, &h_));
    }
    ~TfheLut32() { pfhe_tfhe32_lut_destroy(h_); }
    TfheLut32(const TfheLut32 &) = delete;
    TfheLut32 &operator=(const TfheLut32 &) = delete;
    pfhe_tfhe32_lut_handle *handle() const { return h_; }
    bool in_use() const { return pfhe_tfhe32_lut_in_use(h_) != 0; }
    size_t scratch_bytes() const { return pfhe_tfhe32_lut_scratch_bytes(h_); }
    void rotate_by_bits(const uint32_t *inp, size_t len_inp, const double *keys, size_t len_keys, size_t keys_per_input,
                        size_t first_key, uint32_t *out, size_t len_out) {
        check(pfhe_tfhe32_rotate_by_bits(h_, inp, len_inp, keys, len_keys, keys_per_input, first_key, out, len_out));
    }
    void rotate_by_bits_dev(const uint32_t *inp_dev, size_t len_inp, const double *keys_dev, size_t len_keys,
                            size_t keys_per_input, size_t first_key, uint32_t *out_dev, size_t len_out, void *stream = nullptr) {
        check(pfhe_tfhe32_rotate_by_bits_dev(h_, inp_dev, len_inp, keys_dev, len_keys, keys_per_input, first_key, out_dev, len_out,
                                              stream));
    }
    void lut_eval(const uint32_t *table, size_t len_table, const double *selectors, size_t len_selectors, size_t extract,
                  uint32_t *out, size_t len_out) {
        check(pfhe_tfhe32_lut_eval(h_, table, len_table, selectors, len_selectors, extract, out, len_out));
    }
    void lut_eval_dev(const uint32_t *table_dev, size_t len_table, const double *selectors_dev, size_t len_selectors,
                      size_t extract, uint32_t *out_dev, size_t len_out, void *stream = nullptr) {
        check(pfhe_tfhe32_lut_eval_dev(h_, table_dev, len_table, selectors_dev, len_selectors, extract, out_dev, len_out, stream));
    }

  private:
    pfhe_tfhe32_lut_handle *h_ = nullptr;
};

}  // namespace pfhe
