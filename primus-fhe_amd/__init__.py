"""primus-fhe hot path on MI355X: host-side mirror of the reference's operator interface.

The classes keep the reference's names and argument meaning
(`U64NttTable`, `U64DcrtTable`, ... — primus_ntt / primus_poly / primus_rns / primus_decompose /
primus_lattice) and delegate through the C ABI in include/pfhe.h to hand-written HIP kernels
(csrc/).  There is no CPU fallback: if libpfhe_hip.so is missing or no GPU is visible the
constructors raise.
"""
from ._lib import PfheError, build, lib, library_path, status_string  # noqa: F401
from .lattice import (BlindRotateContext, BlindRotateContext32, blind_rotate, blind_rotate_dev,  # noqa: F401
                      DcrtGlevContext, DcrtGlevContext32, add_dcrt_glev_mul_big_uint_poly_assign_dev,  # noqa: F401
                      add_dcrt_glev_mul_crt_poly_assign_dev, glev_mul_big_uint_poly_to_dev, glev_mul_crt_poly_to_dev,
                      mul_dcrt_ggsw_to, mul_dcrt_ggsw_to_dev, profile_mul_dcrt_ggsw_to_dev)
from .ntt import NttError, U32DcrtTable, U32NttTable, U64DcrtTable, U64NttTable  # noqa: F401
from .tfhe import (ApproxSignedBasis, FullComplex64FftTable, TfheBlindRotateContext, TfheBootstrapContext,  # noqa: F401
                   TfheFftContext, TfheMultiBitBlindRotateContext, glwe_sample_extract, glwe_sample_extract_dev,
                   lwe_keyswitch, lwe_keyswitch_dev, lwe_modulus_switch_dev, lwe_modulus_switch_strided_dev,
                   tfhe_many_lut_test_vector, tfhe_blind_rotate, tfhe_blind_rotate_dev,
                   tfhe_bootstrap, tfhe_bootstrap_dev, tfhe_external_product_to, tfhe_external_product_to_dev,
                   tfhe_multibit_blind_rotate, tfhe_multibit_blind_rotate_dev, tfhe_multibit_combine_key_dev,
                   write_fourier_form, TfheKeyShape, ggsw_add_gadget_dev, glwe_encrypt, glwe_encrypt_dev, glwe_phase,
                   glwe_phase_dev, lwe_encrypt, lwe_encrypt_dev, lwe_phase, lwe_phase_dev, tfhe_generate_bsk_dev,
                   tfhe_generate_ksk_dev, torus_noise, torus_uniform, lwe_pack_keyswitch, lwe_pack_keyswitch_dev,
                   tfhe_generate_pksk_dev, glwe_sample_extract_first_few, glwe_sample_extract_first_few_dev,
                   multimsg_lwe_extract, multimsg_lwe_extract_dev, TfhePackFftContext, tfhe_pack_key_fourier_dev,
                   lwe_pack_keyswitch_fft, lwe_pack_keyswitch_fft_dev, lwe_private_keyswitch, lwe_private_keyswitch_dev,
                   tfhe_generate_pfksk_dev, TfheCircuitBootstrapContext, tfhe_circuit_bootstrap,
                   tfhe_circuit_bootstrap_dev, TfheCmuxTreeContext, tfhe_cmux, tfhe_cmux_dev, tfhe_cmux_tree,
                   tfhe_cmux_tree_dev, TfheGlweTraceContext, glwe_automorphism, glwe_automorphism_dev, glwe_keyswitch,
                   glwe_keyswitch_dev, glwe_trace, glwe_trace_dev, TfheRingPackContext, glwe_ring_merge,
                   glwe_ring_merge_dev, lwe_ring_pack, lwe_ring_pack_dev, tfhe_generate_gksk_dev, lwe_embed_glwe,
                   lwe_embed_glwe_dev, TfheLutContext, tfhe_rotate_by_bits, tfhe_rotate_by_bits_dev, tfhe_lut_eval,
                   tfhe_lut_eval_dev, tfhe_lut_table, TfheBitExtractContext, tfhe_extract_bits, tfhe_extract_bits_dev,
                   tfhe_lut_on_integer_dev, lwe_linear, lwe_linear_dev, tfhe_dense_layer_dev, RandSeed, csprng_keystream_dev,
                   torus_uniform_dev, torus_binary_dev, torus_ternary_dev, torus_tuniform_dev, tfhe_fill_rows_dev,
                   lwe_encrypt_seeded, lwe_encrypt_seeded_dev, seeded_expand, seeded_expand_dev,
                   tfhe_generate_ksk_seeded_dev)
from .rns import (BaseConverter, BaseConverter32, BigUintApproxSignedBasis, BigUintApproxSignedBasis32, RNSBase, RNSBase32,  # noqa: F401
                  RNSError)

__all__ = ["PfheError", "NttError", "RNSError", "U64NttTable", "U64DcrtTable", "U32NttTable", "U32DcrtTable", "RNSBase",
           "BigUintApproxSignedBasis", "BaseConverter", "BaseConverter32", "DcrtGlevContext", "RNSBase32", "BigUintApproxSignedBasis32",
           "DcrtGlevContext32", "mul_dcrt_ggsw_to", "mul_dcrt_ggsw_to_dev",
           "add_dcrt_glev_mul_crt_poly_assign_dev", "glev_mul_crt_poly_to_dev", "add_dcrt_glev_mul_big_uint_poly_assign_dev",
           "glev_mul_big_uint_poly_to_dev", "BlindRotateContext", "BlindRotateContext32", "blind_rotate", "blind_rotate_dev",
           "FullComplex64FftTable", "ApproxSignedBasis", "TfheFftContext", "tfhe_external_product_to",
           "tfhe_external_product_to_dev", "write_fourier_form", "TfheBlindRotateContext", "tfhe_blind_rotate",
           "tfhe_blind_rotate_dev", "lwe_modulus_switch_dev", "lwe_modulus_switch_strided_dev", "tfhe_many_lut_test_vector", "glwe_sample_extract", "glwe_sample_extract_dev",
           "lwe_keyswitch", "lwe_keyswitch_dev", "TfheBootstrapContext", "tfhe_bootstrap", "tfhe_bootstrap_dev",
           "TfheMultiBitBlindRotateContext", "tfhe_multibit_blind_rotate", "tfhe_multibit_blind_rotate_dev",
           "tfhe_multibit_combine_key_dev", "lwe_encrypt", "lwe_encrypt_dev", "lwe_phase", "lwe_phase_dev", "glwe_encrypt",
           "glwe_encrypt_dev", "glwe_phase", "glwe_phase_dev", "ggsw_add_gadget_dev", "TfheKeyShape", "tfhe_generate_bsk_dev",
           "tfhe_generate_ksk_dev", "torus_uniform", "torus_noise", "lwe_pack_keyswitch",
           "lwe_pack_keyswitch_dev", "tfhe_generate_pksk_dev", "glwe_sample_extract_first_few",
           "glwe_sample_extract_first_few_dev", "multimsg_lwe_extract", "multimsg_lwe_extract_dev",
           "TfhePackFftContext", "tfhe_pack_key_fourier_dev", "lwe_pack_keyswitch_fft", "lwe_pack_keyswitch_fft_dev",
           "lwe_private_keyswitch", "lwe_private_keyswitch_dev", "tfhe_generate_pfksk_dev", "TfheCircuitBootstrapContext",
           "tfhe_circuit_bootstrap", "tfhe_circuit_bootstrap_dev", "TfheCmuxTreeContext", "tfhe_cmux", "tfhe_cmux_dev",
           "tfhe_cmux_tree", "tfhe_cmux_tree_dev", "TfheGlweTraceContext", "glwe_automorphism", "glwe_automorphism_dev",
           "glwe_keyswitch", "glwe_keyswitch_dev", "glwe_trace", "glwe_trace_dev", "TfheRingPackContext", "glwe_ring_merge",
           "glwe_ring_merge_dev", "lwe_ring_pack", "lwe_ring_pack_dev", "tfhe_generate_gksk_dev", "lwe_embed_glwe",
           "lwe_embed_glwe_dev", "TfheLutContext", "tfhe_rotate_by_bits", "tfhe_rotate_by_bits_dev", "tfhe_lut_eval",
           "tfhe_lut_eval_dev", "tfhe_lut_table", "TfheBitExtractContext", "tfhe_extract_bits", "tfhe_extract_bits_dev",
           "tfhe_lut_on_integer_dev", "lwe_linear", "lwe_linear_dev", "tfhe_dense_layer_dev", "RandSeed",
           "csprng_keystream_dev", "torus_uniform_dev", "torus_binary_dev", "torus_ternary_dev", "torus_tuniform_dev",
           "tfhe_fill_rows_dev", "lwe_encrypt_seeded", "lwe_encrypt_seeded_dev", "seeded_expand", "seeded_expand_dev",
           "tfhe_generate_ksk_seeded_dev", "build", "lib", "library_path", "status_string"]
