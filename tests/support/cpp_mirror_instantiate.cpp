// Compile coverage of include/pfhe.hpp, compiled only and never run: every class template instantiated for both word
// types, every free function template called once per word type, and the alias pairs pinned to their C handle types.
// tests/test_cpp_header.py compares the pfhe_* symbols this unit leaves undefined with cpp_mirror_symbols.txt.
#include <type_traits>
#include <utility>

#include "pfhe.hpp"

namespace pfhe {
template class RNSBaseT<uint64_t>;
template class RNSBaseT<uint32_t>;
template class BaseConverterT<uint64_t>;
template class BaseConverterT<uint32_t>;
template class BigUintApproxSignedBasisT<uint64_t>;
template class BigUintApproxSignedBasisT<uint32_t>;
template class DcrtGlevContextT<uint64_t>;
template class DcrtGlevContextT<uint32_t>;
template class BlindRotateT<uint64_t>;
template class BlindRotateT<uint32_t>;
template class TfheFftContextT<uint64_t>;
template class TfheFftContextT<uint32_t>;
template class TfheBlindRotateT<uint64_t>;
template class TfheBlindRotateT<uint32_t>;
template class TfheMultiBitBlindRotateT<uint64_t>;
template class TfheMultiBitBlindRotateT<uint32_t>;
template class TfheBootstrapT<uint64_t>;
template class TfheBootstrapT<uint32_t>;
template class TfhePackFftContextT<uint64_t>;
template class TfhePackFftContextT<uint32_t>;
template class TfheCircuitBootstrapT<uint64_t>;
template class TfheCircuitBootstrapT<uint32_t>;
template class TfheCmuxTreeT<uint64_t>;
template class TfheCmuxTreeT<uint32_t>;
template class TfheGlweTraceT<uint64_t>;
template class TfheGlweTraceT<uint32_t>;
template class TfheLutT<uint64_t>;
template class TfheLutT<uint32_t>;
}  // namespace pfhe

// the two public names of a class are two types, and handle() gives the C handle of each width
#define MIRROR_PAIR(NAME, H64, H32)                                                                          \
    static_assert(!std::is_same<pfhe::NAME, pfhe::NAME##32>::value, #NAME " and " #NAME "32 are one type");  \
    static_assert(std::is_same<decltype(std::declval<const pfhe::NAME &>().handle()), H64>::value, #NAME);   \
    static_assert(std::is_same<decltype(std::declval<const pfhe::NAME##32 &>().handle()), H32>::value, #NAME "32")
MIRROR_PAIR(RNSBase, const pfhe_rns *, const pfhe_rns32 *);
MIRROR_PAIR(BaseConverter, const pfhe_conv *, const pfhe_conv32 *);
MIRROR_PAIR(BigUintApproxSignedBasis, const pfhe_basis *, const pfhe_basis32 *);
MIRROR_PAIR(DcrtGlevContext, pfhe_extprod_plan *, pfhe_extprod32_plan *);
MIRROR_PAIR(BlindRotate, pfhe_blindrot *, pfhe_blindrot32 *);
MIRROR_PAIR(TfheFftContext, pfhe_tfhe_plan *, pfhe_tfhe32_plan *);
MIRROR_PAIR(TfheBlindRotate, pfhe_tfhe_blindrot *, pfhe_tfhe32_blindrot *);
MIRROR_PAIR(TfheMultiBitBlindRotate, pfhe_tfhe_mbrot *, pfhe_tfhe32_mbrot *);
MIRROR_PAIR(TfheBootstrap, pfhe_tfhe_bootstrap_handle *, pfhe_tfhe32_bootstrap_handle *);
MIRROR_PAIR(TfhePackFftContext, pfhe_tfhe_packfft_plan *, pfhe_tfhe32_packfft_plan *);
MIRROR_PAIR(TfheCircuitBootstrap, pfhe_tfhe_cbs_handle *, pfhe_tfhe32_cbs_handle *);
MIRROR_PAIR(TfheCmuxTree, pfhe_tfhe_cmux_tree_handle *, pfhe_tfhe32_cmux_tree_handle *);
MIRROR_PAIR(TfheGlweTrace, pfhe_tfhe_glwe_trace_handle *, pfhe_tfhe32_glwe_trace_handle *);
MIRROR_PAIR(TfheLut, pfhe_tfhe_lut_handle *, pfhe_tfhe32_lut_handle *);
#undef MIRROR_PAIR
static_assert(std::is_same<decltype(std::declval<const pfhe::FullComplex64FftTable &>().handle()), pfhe_fft *>::value, "fft");
static_assert(std::is_same<decltype(std::declval<const pfhe::U64DcrtTable &>().handle()), const pfhe_dcrt *>::value, "dcrt");
static_assert(std::is_same<decltype(std::declval<const pfhe::U32DcrtTable &>().handle()), const pfhe_dcrt32 *>::value, "dcrt32");
static_assert(std::is_move_constructible<pfhe::TfheLut>::value && !std::is_copy_constructible<pfhe::TfheLut>::value &&
                  !std::is_copy_assignable<pfhe::TfheLut32>::value && std::is_move_constructible<pfhe::U64NttTable>::value,
              "handles move and do not copy");

// What the classes inherit from their owner is instantiated by use: in_use() and scratch_bytes() of every handle that has
// them.  The u64 DcrtGlevContext has no scratch_bytes().
template <class W>
size_t every_inherited_call(const pfhe::DcrtGlevContextT<W> &glev, const pfhe::BlindRotateT<W> &rot,
                            const pfhe::TfheFftContextT<W> &ctx, const pfhe::TfheBlindRotateT<W> &trot,
                            const pfhe::TfheMultiBitBlindRotateT<W> &mb, const pfhe::TfheBootstrapT<W> &bs,
                            const pfhe::TfhePackFftContextT<W> &pack, const pfhe::TfheCircuitBootstrapT<W> &cbs,
                            const pfhe::TfheCmuxTreeT<W> &cmux, const pfhe::TfheGlweTraceT<W> &trace,
                            const pfhe::TfheLutT<W> &lut) {
    size_t bytes = 0;
    if constexpr (std::is_same<W, uint32_t>::value) bytes += glev.scratch_bytes();
    const bool busy = glev.in_use() || rot.in_use() || ctx.in_use() || trot.in_use() || mb.in_use() || bs.in_use() ||
                      pack.in_use() || cbs.in_use() || cmux.in_use() || trace.in_use() || lut.in_use();
    return busy ? 0
                : bytes + rot.scratch_bytes() + ctx.scratch_bytes() + trot.scratch_bytes() + mb.scratch_bytes() +
                      bs.scratch_bytes() + pack.scratch_bytes() + cbs.scratch_bytes() + cmux.scratch_bytes() +
                      trace.scratch_bytes() + lut.scratch_bytes();
}
template size_t every_inherited_call<uint64_t>(const pfhe::DcrtGlevContext &, const pfhe::BlindRotate &,
                                               const pfhe::TfheFftContext &, const pfhe::TfheBlindRotate &,
                                               const pfhe::TfheMultiBitBlindRotate &, const pfhe::TfheBootstrap &,
                                               const pfhe::TfhePackFftContext &, const pfhe::TfheCircuitBootstrap &,
                                               const pfhe::TfheCmuxTree &, const pfhe::TfheGlweTrace &, const pfhe::TfheLut &);
template size_t every_inherited_call<uint32_t>(const pfhe::DcrtGlevContext32 &, const pfhe::BlindRotate32 &,
                                               const pfhe::TfheFftContext32 &, const pfhe::TfheBlindRotate32 &,
                                               const pfhe::TfheMultiBitBlindRotate32 &, const pfhe::TfheBootstrap32 &,
                                               const pfhe::TfhePackFftContext32 &, const pfhe::TfheCircuitBootstrap32 &,
                                               const pfhe::TfheCmuxTree32 &, const pfhe::TfheGlweTrace32 &,
                                               const pfhe::TfheLut32 &);

// Every free function template once.  `w` is a non-const buffer and `cw` a const one: both go where `const W *` is taken,
// and a literal nullptr goes where a buffer is optional to the caller, as with the plain overloads these templates replace.
template <class W>
void every_free_function(const pfhe::FullComplex64FftTable &fft, pfhe::DcrtGlevContextT<W> &glev, pfhe::TfheFftContextT<W> &ctx,
                         pfhe::TfhePackFftContextT<W> &pack, W *w, const W *cw, double *d, uint32_t *e, void *stream) {
    const double *cd = d;
    const uint32_t *ce = e;
    pfhe::mul_dcrt_ggsw_to(cw, 1, w, 1, w, 1, glev);
    pfhe::mul_dcrt_ggsw_to(w, 1, cw, 1, w, 1, glev, true);
    pfhe::mul_dcrt_ggsw_to_dev(cw, 1, w, 1, w, 1, glev);
    pfhe::mul_dcrt_ggsw_to_dev(w, 1, cw, 1, w, 1, glev, true, stream);
    pfhe::external_product_to(cw, 1, cd, 1, w, 1, ctx);
    pfhe::external_product_to(w, 1, d, 1, w, 1, ctx);
    pfhe::external_product_to_dev(cw, 1, cd, 1, w, 1, ctx);
    pfhe::external_product_to_dev(w, 1, d, 1, w, 1, ctx, stream);
    pfhe::mul_monomial_each_to_dev(fft, cw, 1, ce, 1, w);
    pfhe::mul_monomial_each_to_dev(fft, w, 1, e, 1, w, stream);
    pfhe::lwe_modulus_switch_dev(0, cw, 1, 1, 3, e, 1, e, 1);
    pfhe::lwe_modulus_switch_dev(0, w, 1, 1, 3, e, 1, e, 1, stream);
    pfhe::lwe_modulus_switch_strided_dev(0, cw, 1, 1, 3, 1, e, 1, e, 1);
    pfhe::lwe_modulus_switch_strided_dev(0, w, 1, 1, 3, 1, e, 1, e, 1, stream);
    pfhe::glwe_sample_extract(fft, 1, cw, 1, 0, w, 1);
    pfhe::glwe_sample_extract(fft, 1, w, 1, 0, w, 1);
    pfhe::glwe_sample_extract_dev(fft, 1, cw, 1, 0, w, 1);
    pfhe::glwe_sample_extract_dev(fft, 1, w, 1, 0, w, 1, stream);
    pfhe::lwe_keyswitch(0, cw, 1, 1, cw, 1, 1, 8, 0, w, 1);
    pfhe::lwe_keyswitch(0, w, 1, 1, w, 1, 1, 8, 0, w, 1);
    pfhe::lwe_keyswitch(0, w, 1, 1, nullptr, 0, 1, 8, 0, w, 1);
    pfhe::lwe_keyswitch_dev(0, cw, 1, 1, cw, 1, 1, 8, 0, w, 1);
    pfhe::lwe_keyswitch_dev(0, w, 1, 1, w, 1, 1, 8, 0, w, 1, stream);
    pfhe::lwe_keyswitch_dev(0, w, 1, 1, nullptr, 0, 1, 8, 0, w, 1, nullptr);
    pfhe::lwe_body_mac(0, w, 1, 1, cw, 1, false);
    pfhe::lwe_body_mac(0, w, 1, 1, w, 1, true);
    pfhe::lwe_body_mac_dev(0, w, 1, 1, cw, 1, false);
    pfhe::lwe_body_mac_dev(0, w, 1, 1, w, 1, true, stream);
    pfhe::glwe_body_mac(fft, 1, w, 1, cw, 1, false);
    pfhe::glwe_body_mac(fft, 1, w, 1, w, 1, true);
    pfhe::glwe_body_mac_dev(fft, 1, w, 1, cw, 1, false);
    pfhe::glwe_body_mac_dev(fft, 1, w, 1, w, 1, true, stream);
    pfhe::ggsw_add_gadget_dev(fft, 1, 8, 2, w, 1, cw, 1);
    pfhe::ggsw_add_gadget_dev(fft, 1, 8, 2, w, 1, w, 1, stream);
    pfhe::tfhe_generate_bsk_dev(fft, 1, 8, 2, 0, cw, 1, cw, 1, w, 1, d, 1);
    pfhe::tfhe_generate_bsk_dev(fft, 1, 8, 2, 0, w, 1, w, 1, w, 1, d, 1, stream);
    pfhe::tfhe_generate_ksk_dev(0, cw, 1, cw, 1, 8, 2, w, 1);
    pfhe::tfhe_generate_ksk_dev(0, w, 1, w, 1, 8, 2, w, 1, stream);
    pfhe::lwe_pack_keyswitch(fft, 1, cw, 1, 1, 1, cw, 1, 8, 2, w, 1);
    pfhe::lwe_pack_keyswitch(fft, 1, w, 1, 1, 1, w, 1, 8, 2, w, 1);
    pfhe::lwe_pack_keyswitch_dev(fft, 1, cw, 1, 1, 1, cw, 1, 8, 2, w, 1);
    pfhe::lwe_pack_keyswitch_dev(fft, 1, w, 1, 1, 1, w, 1, 8, 2, w, 1, stream);
    pfhe::tfhe_generate_pksk_dev(fft, 1, cw, 1, cw, 1, 8, 2, w, 1);
    pfhe::tfhe_generate_pksk_dev(fft, 1, w, 1, w, 1, 8, 2, w, 1, stream);
    pfhe::glwe_sample_extract_first_few(fft, 1, cw, 1, 1, w, 1);
    pfhe::glwe_sample_extract_first_few(fft, 1, w, 1, 1, w, 1);
    pfhe::glwe_sample_extract_first_few_dev(fft, 1, cw, 1, 1, w, 1);
    pfhe::glwe_sample_extract_first_few_dev(fft, 1, w, 1, 1, w, 1, stream);
    pfhe::multimsg_lwe_extract(fft, 1, cw, 1, 1, w, 1);
    pfhe::multimsg_lwe_extract(fft, 1, w, 1, 1, w, 1);
    pfhe::multimsg_lwe_extract_dev(fft, 1, cw, 1, 1, w, 1);
    pfhe::multimsg_lwe_extract_dev(fft, 1, w, 1, 1, w, 1, stream);
    pfhe::tfhe_pack_key_fourier_dev(cw, 1, d, 1, pack);
    pfhe::tfhe_pack_key_fourier_dev(w, 1, d, 1, pack, stream);
    pfhe::lwe_pack_keyswitch_fft(cw, 1, 1, cd, 1, w, 1, pack);
    pfhe::lwe_pack_keyswitch_fft(w, 1, 1, d, 1, w, 1, pack);
    pfhe::lwe_pack_keyswitch_fft_dev(cw, 1, 1, cd, 1, w, 1, pack);
    pfhe::lwe_pack_keyswitch_fft_dev(w, 1, 1, d, 1, w, 1, pack, stream);
    pfhe::lwe_private_keyswitch(fft, 1, cw, 1, 1, 1, cw, 1, 8, 2, w, 1);
    pfhe::lwe_private_keyswitch(fft, 1, w, 1, 1, 1, w, 1, 8, 2, w, 1);
    pfhe::lwe_private_keyswitch_dev(fft, 1, cw, 1, 1, 1, cw, 1, 8, 2, w, 1);
    pfhe::lwe_private_keyswitch_dev(fft, 1, w, 1, 1, 1, w, 1, 8, 2, w, 1, stream);
    pfhe::tfhe_generate_pfksk_dev(fft, 1, cw, 1, cw, 1, 8, 2, w, 1);
    pfhe::tfhe_generate_pfksk_dev(fft, 1, w, 1, w, 1, 8, 2, w, 1, stream);
    // the four member templates of the table, and the method that takes an optional key
    fft.forward_torus_slice(cw, 1, d, 1);
    fft.forward_torus_slice(w, 1, d, 1);
    fft.inverse_torus_slice(cd, 1, w, 1);
    fft.forward_torus_dev(cw, 1, d, 1);
    fft.forward_torus_dev(w, 1, d, 1, stream);
    fft.inverse_torus_dev(cd, 1, w, 1);
    fft.inverse_torus_dev(d, 1, w, 1, stream);
    pfhe::TfheBootstrapT<W> bs(fft, 1, 8, 2, 4, 4, 2, false);
    bs.bootstrap(w, 1, d, 1, w, 1, nullptr, 0, w, 1);
    bs.bootstrap_dev(cw, 1, cd, 1, cw, 1, nullptr, 0, w, 1);
    pfhe::tfhe_multibit_combine_key_dev(fft, 1, 2, 2, cd, 1, ce, 1, d, 1);
}
template void every_free_function<uint64_t>(const pfhe::FullComplex64FftTable &, pfhe::DcrtGlevContext &, pfhe::TfheFftContext &,
                                            pfhe::TfhePackFftContext &, uint64_t *, const uint64_t *, double *, uint32_t *,
                                            void *);
template void every_free_function<uint32_t>(const pfhe::FullComplex64FftTable &, pfhe::DcrtGlevContext32 &,
                                            pfhe::TfheFftContext32 &, pfhe::TfhePackFftContext32 &, uint32_t *,
                                            const uint32_t *, double *, uint32_t *, void *);
