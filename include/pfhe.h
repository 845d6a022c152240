/*
 * pfhe.h — C ABI of the MI355X-native polynomial-ring engine (libpfhe_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of primus-labs/primus-fhe: negacyclic NTT/INTT
 * over 64-bit primes, RNS ("DCRT") pointwise arithmetic, and the RNS gadget external product.
 * The reference has no FFI of its own; the seam is the pair of Rust traits `NttTable` /
 * `DcrtTable` plus the slice-level functions of primus_poly / primus_rns / primus_decompose /
 * primus_lattice that are generic over them.  Every entry point below names the reference item
 * (file:line under /root/reference/crates/) it replaces; INTEGRATION.md shows the Rust binding.
 *
 * Conventions
 *   - plain pointers + sizes, no C++/torch types; every function returns a pfhe_status (0 = OK)
 *     and never aborts or throws across the boundary (the reference panics / debug_asserts).
 *   - words are uint64_t; layouts are the reference's: a polynomial is N contiguous words, an
 *     RNS polynomial is L x N words modulus-major (primus_rns/src/lib.rs:12-16), batches are
 *     plain concatenation.  `len` is always the TOTAL number of words and must be a multiple of
 *     the unit size (the reference only debug_asserts lengths; we return PFHE_ERR_BAD_LENGTH).
 *   - `*_slice` functions take HOST pointers and behave exactly like the reference call
 *     (in place, synchronous).  `*_dev` functions take DEVICE pointers that live on the handle's
 *     GPU plus a hipStream_t (as void*, NULL = default stream); they are asynchronous and are
 *     the measured hot path.  Device buffers must be 16-byte aligned (PFHE_ERR_BAD_ARGUMENT
 *     otherwise; hipMalloc / pfhe_device_malloc memory always is).
 *   - handles are immutable after creation and may be shared between host threads
 *     (NttTable: Send + Sync, primus_ntt/src/ntt/mod.rs:16); an external-product plan owns
 *     scratch and has one holder at a time (it mirrors `&mut DcrtGlevContext`,
 *     primus_lattice/src/context/glev.rs:4-10): a call from a second thread while one is inside
 *     is refused with PFHE_ERR_BUSY, not raced.
 *   - there is NO CPU fallback: without a HIP device create() fails with PFHE_ERR_NO_DEVICE.
 */
#ifndef PFHE_H
#define PFHE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: 1..5 mirror NttError (primus_ntt/src/error.rs:7-49), 16..18 RNSError
 *      (primus_rns/src/lib.rs), 32.. are boundary errors the reference cannot have. ---- */
typedef enum pfhe_status {
    PFHE_OK = 0,
    PFHE_ERR_NO_PRIMITIVE_ROOT = 1,
    PFHE_ERR_DEGREE_CONVERSION = 2,
    PFHE_ERR_DEGREE_TOO_LARGE = 3,
    PFHE_ERR_NTT_TABLE = 4,
    PFHE_ERR_MODULUS_TOO_LARGE = 5,
    PFHE_ERR_EMPTY_BASE = 16,
    PFHE_ERR_COPRIME = 17,
    PFHE_ERR_UNREPRESENTABLE_MODULUS = 18,
    PFHE_ERR_BAD_LENGTH = 32,
    PFHE_ERR_BAD_ARGUMENT = 33,
    PFHE_ERR_NO_DEVICE = 34,
    PFHE_ERR_HIP = 35,
    PFHE_ERR_UNSUPPORTED = 36,
    PFHE_ERR_NO_INVERSE = 37, /* ReduceError::NoInverse: an element of an inversion is not a unit */
    PFHE_ERR_BUSY = 38        /* an external-product plan is held by another thread (one holder at a time) */
} pfhe_status;

const char *pfhe_status_string(int status);
/* Thread-local detail of the last failure on this thread (e.g. the HIP error string). */
const char *pfhe_last_error(void);
/* "libpfhe_hip <version> gfx950" */
const char *pfhe_version(void);

/* ---- device plumbing (so a Rust/C caller needs no HIP headers) ---- */
int pfhe_device_count(int *count);
int pfhe_device_malloc(int device, size_t bytes, void **out);
int pfhe_device_free(int device, void *ptr);
int pfhe_memcpy_h2d(int device, void *dst_dev, const void *src_host, size_t bytes, void *stream);
int pfhe_memcpy_d2h(int device, void *dst_host, const void *src_dev, size_t bytes, void *stream);
int pfhe_memcpy_d2d(int device, void *dst_dev, const void *src_dev, size_t bytes, void *stream);
int pfhe_memset_dev(int device, void *dst_dev, int byte, size_t bytes, void *stream);
/* Measurement aid (bench.py `device_copy`): a copy by a kernel of the element-wise family's launch shape — one 16-byte vector
 * per thread, non-temporal loads and stores; `bytes` a multiple of 16, both pointers 16-byte aligned, ranges disjoint. */
int pfhe_stream_copy_dev(int device, void *dst_dev, const void *src_dev, size_t bytes, void *stream);
int pfhe_stream_synchronize(int device, void *stream);
/* Host-pointer entry points (`*_slice`, `*_to` without `_dev`) behave like the reference's `&self, &mut [T]` methods
 * (table.rs:541-563: in place, no allocation per call): each call borrows a staging context — private streams, cached
 * device arena, pinned host buffer — from a per-device pool and returns it, so calls of a size seen before allocate
 * nothing and any number of threads may call through one handle concurrently (NttTable: Send + Sync).
 * pfhe_debug_alloc_count: device / pinned allocation and free calls the library has made since it was loaded (a
 * steady-state loop must not move it).  pfhe_staging_release: frees the idle contexts of `device` (-1: all devices),
 * returns their number (at most four are kept per device anyway).
 * pfhe_debug_stage_path_count(which): host-pointer calls that took path `which` since the library was loaded —
 * 0 kernels on pinned memory the caller ALLOCATED (hipHostMalloc, a torch pinned tensor), 1 kernels on the pool's own pinned
 * buffer (pageable slices, and since round 5 slices the caller merely REGISTERED with hipHostRegister: kernels running on a
 * per-call registration return rare wrong words on this platform with plain HIP alone — tools/microbench12_register_hazard.hip),
 * 2 copy engines on caller-pinned memory (allocated or registered), 3 the runtime's pageable copies, 4 long pageable slices
 * with the copy back on the context's helper thread, 5 small uploads of the non-transform entry points: a CPU copy into the
 * pool's pinned buffer + a copy-engine transfer.
 * Every entry point clears the calling thread's pending HIP error (hipGetLastError is sticky per thread) on the way in — the
 * outermost one of a call only — so that an earlier failed HIP call of the caller's own is not reported as a failure of
 * this library's launches: check the return values of your own HIP calls, not hipGetLastError after a pfhe_* call.
 * Streams: since round 4 the host-pointer entry points run on PRIVATE non-blocking streams of the borrowed context, not on
 * the legacy null stream: they are ordered with respect to nothing the caller has queued elsewhere (they block until
 * their own work is done, which is all `&mut [T]` semantics need). */
uint64_t pfhe_debug_alloc_count(void);
uint64_t pfhe_debug_stage_path_count(int which);
int pfhe_staging_release(int device);
/* Synthetic data: word i of the buffer = floor(splitmix64(seed, i) * q / 2^64), i.e. uniform in
 * [0,q) (per-modulus uniform sampling as primus_distr/src/common.rs:244-263).  Modulus-major RNS
 * layout when `moduli_count` > 1: word i uses moduli[(i / poly_len) % moduli_count]. */
int pfhe_fill_uniform_dev(int device, uint64_t *dst_dev, size_t len, const uint64_t *moduli,
                          size_t moduli_count, size_t poly_len, uint64_t seed, void *stream);

/* =====================================================================================
 * U64NttTable — primus_ntt/src/ntt/prime64/table.rs:41 implementing NttTable
 * (primus_ntt/src/ntt/mod.rs:16-113)
 * ===================================================================================== */
typedef struct pfhe_ntt pfhe_ntt;

/* NttTable::new(log_n, modulus) — table.rs:308-516.  Errors: NO_PRIMITIVE_ROOT when 2N does not
 * divide q-1 (root.rs:76-81), MODULUS_TOO_LARGE when q >= 2^62 (table.rs:318-323). */
int pfhe_ntt_create(uint32_t log_n, uint64_t modulus, int device, pfhe_ntt **out);
void pfhe_ntt_destroy(pfhe_ntt *table);
/* getters — table.rs:127-161, ntt/mod.rs:26 (poly_length) */
size_t pfhe_ntt_poly_length(const pfhe_ntt *table);
uint32_t pfhe_ntt_log_n(const pfhe_ntt *table);
uint64_t pfhe_ntt_modulus(const pfhe_ntt *table);
uint64_t pfhe_ntt_root(const pfhe_ntt *table);
uint64_t pfhe_ntt_inv_root(const pfhe_ntt *table);
uint64_t pfhe_ntt_inv_n(const pfhe_ntt *table);
int pfhe_ntt_device(const pfhe_ntt *table);

/* transform_slice / inverse_transform_slice / lazy_* — table.rs:541-563.  `len` = batch * N;
 * each N-word chunk is transformed independently in place.
 *   forward: normal order in, bit-reversed out; canonical [0,q) (lazy: [0,4q) in and out)
 *   inverse: bit-reversed in, normal order out; canonical [0,q) (lazy: [0,2q) in and out) */
int pfhe_ntt_transform_slice(const pfhe_ntt *table, uint64_t *poly, size_t len);
int pfhe_ntt_inverse_transform_slice(const pfhe_ntt *table, uint64_t *values, size_t len);
int pfhe_ntt_lazy_transform_slice(const pfhe_ntt *table, uint64_t *poly, size_t len);
int pfhe_ntt_lazy_inverse_transform_slice(const pfhe_ntt *table, uint64_t *values, size_t len);
/* transform_monomial / transform_coeff_one_monomial / transform_coeff_minus_one_monomial —
 * table.rs:565-651.  `values` receives N words. */
int pfhe_ntt_transform_monomial(const pfhe_ntt *table, uint64_t coeff, size_t degree,
                                uint64_t *values, size_t len);
int pfhe_ntt_transform_coeff_one_monomial(const pfhe_ntt *table, size_t degree, uint64_t *values,
                                          size_t len);
int pfhe_ntt_transform_coeff_minus_one_monomial(const pfhe_ntt *table, size_t degree,
                                                uint64_t *values, size_t len);
/* device-pointer variants (hot path).  lazy != 0 selects the lazy_* contract. */
int pfhe_ntt_transform_dev(const pfhe_ntt *table, uint64_t *poly_dev, size_t len, int lazy,
                           void *stream);
int pfhe_ntt_inverse_transform_dev(const pfhe_ntt *table, uint64_t *values_dev, size_t len,
                                   int lazy, void *stream);
int pfhe_ntt_transform_monomial_dev(const pfhe_ntt *table, uint64_t coeff, size_t degree,
                                    uint64_t *values_dev, size_t len, void *stream);
/* NttPolynomial::mul_assign / add_mul_assign — primus_poly/src/ntt/mul.rs:84-90,
 * ntt/mod.rs:101-112 (-> reduce_mul_slice_assign / reduce_add_mul_slice_assign,
 * primus_modulus/src/common/compact/slice.rs:106-115,210-221).  len_b is len_a (elementwise)
 * or N (one multiplicand shared by the whole batch). */
int pfhe_ntt_mul_assign_dev(const pfhe_ntt *table, uint64_t *a_dev, size_t len_a,
                            const uint64_t *b_dev, size_t len_b, void *stream);
int pfhe_ntt_add_mul_assign_dev(const pfhe_ntt *table, uint64_t *acc_dev, const uint64_t *a_dev,
                                size_t len_a, const uint64_t *b_dev, size_t len_b, void *stream);
/* NttPolynomial::mul_to / mul_add_to — primus_poly/src/ntt/mul.rs:100-107, ntt/mod.rs:169-187:
 * out = a*b and out = a*b + c (out may alias an input). */
int pfhe_ntt_mul_to_dev(const pfhe_ntt *table, const uint64_t *a_dev, size_t len_a,
                        const uint64_t *b_dev, size_t len_b, uint64_t *out_dev, void *stream);
int pfhe_ntt_mul_add_to_dev(const pfhe_ntt *table, const uint64_t *a_dev, size_t len_a,
                            const uint64_t *b_dev, size_t len_b, const uint64_t *c_dev,
                            uint64_t *out_dev, void *stream);

/* =====================================================================================
 * U64DcrtTable — primus_ntt/src/dcrt/prime64.rs:11 implementing DcrtTable
 * (primus_ntt/src/dcrt/mod.rs:19-135).  Unit = one RNS polynomial = L*N words, modulus-major.
 * ===================================================================================== */
typedef struct pfhe_dcrt pfhe_dcrt;

/* DcrtTable::new(log_n, moduli) — dcrt/prime64.rs:24-43 (per-limb NttTable::new errors). */
int pfhe_dcrt_create(uint32_t log_n, const uint64_t *moduli, size_t moduli_count, int device,
                     pfhe_dcrt **out);
void pfhe_dcrt_destroy(pfhe_dcrt *table);
size_t pfhe_dcrt_poly_length(const pfhe_dcrt *table);     /* dcrt/prime64.rs:56 */
size_t pfhe_dcrt_moduli_count(const pfhe_dcrt *table);    /* :61 */
size_t pfhe_dcrt_crt_poly_length(const pfhe_dcrt *table); /* :66 */
int pfhe_dcrt_device(const pfhe_dcrt *table);
/* ntt_tables()[i] getters (dcrt/prime64.rs:46) */
uint64_t pfhe_dcrt_modulus(const pfhe_dcrt *table, size_t i);
uint64_t pfhe_dcrt_root(const pfhe_dcrt *table, size_t i);
uint64_t pfhe_dcrt_inv_n(const pfhe_dcrt *table, size_t i);

/* transform_slice / inverse_transform_slice / lazy_* — dcrt/prime64.rs:98-127.
 * `len` = batch * L * N. */
int pfhe_dcrt_transform_slice(const pfhe_dcrt *table, uint64_t *poly, size_t len);
int pfhe_dcrt_inverse_transform_slice(const pfhe_dcrt *table, uint64_t *poly, size_t len);
int pfhe_dcrt_lazy_transform_slice(const pfhe_dcrt *table, uint64_t *poly, size_t len);
int pfhe_dcrt_lazy_inverse_transform_slice(const pfhe_dcrt *table, uint64_t *poly, size_t len);
/* DcrtTable::transform_monomial & co — dcrt/mod.rs:105-134.  `values` receives L*N words. */
int pfhe_dcrt_transform_monomial(const pfhe_dcrt *table, uint64_t coeff, size_t degree,
                                 uint64_t *values, size_t len);
/* transform_coeff_one_monomial / transform_coeff_minus_one_monomial — dcrt/mod.rs:113-134
 * (-X^degree uses q_i - 1 in limb i). */
int pfhe_dcrt_transform_coeff_one_monomial(const pfhe_dcrt *table, size_t degree, uint64_t *values,
                                           size_t len);
int pfhe_dcrt_transform_coeff_minus_one_monomial(const pfhe_dcrt *table, size_t degree,
                                                 uint64_t *values, size_t len);
/* device-pointer variants of the three monomial transforms: launches on `stream` only (the per-limb coefficients
 * travel as kernel arguments), no allocation or synchronisation — capturable into a HIP graph (a CMUX / blind-rotate
 * loop builds X^d in NTT form every step).  minus_one != 0 selects -X^degree (coeff is then ignored). */
int pfhe_dcrt_transform_monomial_dev(const pfhe_dcrt *table, uint64_t coeff, size_t degree,
                                     uint64_t *values_dev, size_t len, int minus_one, void *stream);
int pfhe_dcrt_transform_dev(const pfhe_dcrt *table, uint64_t *poly_dev, size_t len, int lazy,
                            void *stream);
int pfhe_dcrt_inverse_transform_dev(const pfhe_dcrt *table, uint64_t *poly_dev, size_t len,
                                    int lazy, void *stream);
/* DcrtPolynomial::mul_assign (primus_poly/src/dcrt/mul.rs:176-187) and add_mul_assign
 * (primus_poly/src/dcrt/mod.rs:105-123): per limb Barrett a = a*b, acc = a*b + acc, canonical
 * inputs and outputs.  len_b is len_a or L*N (shared multiplicand). */
int pfhe_dcrt_mul_assign_dev(const pfhe_dcrt *table, uint64_t *a_dev, size_t len_a,
                             const uint64_t *b_dev, size_t len_b, void *stream);
int pfhe_dcrt_add_mul_assign_dev(const pfhe_dcrt *table, uint64_t *acc_dev,
                                 const uint64_t *a_dev, size_t len_a, const uint64_t *b_dev,
                                 size_t len_b, void *stream);
/* DcrtGlwe::add_dcrt_glwe_mul_dcrt_polynomial_assign — primus_lattice/src/glwe/dcrt.rs:107-126,
 * batched: acc and dcrt_glwe hold batch ciphertexts of `glwe_polys` (= k+1) RNS polynomials,
 * dcrt_poly one RNS polynomial per ciphertext (len_poly = len / glwe_polys):
 * acc[e][c] += dcrt_glwe[e][c] * dcrt_poly[e]. */
int pfhe_dcrt_add_dcrt_glwe_mul_dcrt_polynomial_assign_dev(const pfhe_dcrt *table,
                                                           uint64_t *acc_dev,
                                                           const uint64_t *dcrt_glwe_dev, size_t len,
                                                           const uint64_t *dcrt_poly_dev,
                                                           size_t len_poly, size_t glwe_polys,
                                                           void *stream);
/* DcrtGlwe::mul_dcrt_polynomial_to — glwe/dcrt.rs:377-395, batched the same way:
 * result[e][c] = dcrt_glwe[e][c] * dcrt_poly[e]; result may alias dcrt_glwe. */
int pfhe_dcrt_glwe_mul_dcrt_polynomial_to_dev(const pfhe_dcrt *table, const uint64_t *dcrt_glwe_dev, size_t len,
                                              const uint64_t *dcrt_poly_dev, size_t len_poly, size_t glwe_polys,
                                              uint64_t *result_dev, void *stream);
/* DcrtPolynomial::mul_to (primus_poly/src/dcrt/mul.rs:232-250) and the out-of-place
 * multiply-add: out = a*b, out = a*b + c (out may alias an input). */
int pfhe_dcrt_mul_to_dev(const pfhe_dcrt *table, const uint64_t *a_dev, size_t len_a,
                         const uint64_t *b_dev, size_t len_b, uint64_t *out_dev, void *stream);
int pfhe_dcrt_mul_add_to_dev(const pfhe_dcrt *table, const uint64_t *a_dev, size_t len_a,
                             const uint64_t *b_dev, size_t len_b, const uint64_t *c_dev,
                             uint64_t *out_dev, void *stream);
/* GLWE butterfly (self, result) = (self + rhs, (self_orig - rhs) * w), canonical in and out, over
 * every DCRT polynomial of a (batch of) DcrtGlwe:
 *   DcrtGlwe::butterfly_mul_dcrt_polynomial_to — primus_lattice/src/glwe/dcrt.rs:128-155
 *     (-> DcrtPolynomial::butterfly_mul_to, primus_poly/src/dcrt/mod.rs:125-160); w = len_w plain
 *     residues: one DCRT polynomial (L*N, shared by all components) or len.
 *   DcrtGlwe::butterfly_mul_factor_to — glwe/dcrt.rs:157-175 (-> DcrtPolynomial::butterfly_mul_factor_to,
 *     primus_poly/src/dcrt/mul.rs:15-30,196-222); w = ShoupFactor<u64> pairs (value, quotient),
 *     len_w = 2*L*N (shared) or 2*len words. */
int pfhe_dcrt_butterfly_mul_dcrt_polynomial_to_dev(const pfhe_dcrt *table, uint64_t *a_dev,
                                                   const uint64_t *rhs_dev, size_t len,
                                                   const uint64_t *dcrt_poly_dev, size_t len_w,
                                                   uint64_t *result_dev, void *stream);
int pfhe_dcrt_butterfly_mul_factor_to_dev(const pfhe_dcrt *table, uint64_t *a_dev,
                                          const uint64_t *rhs_dev, size_t len,
                                          const uint64_t *factor_poly_dev, size_t len_w,
                                          uint64_t *result_dev, void *stream);
/* Fused "NTT -> pointwise mul by dcrt_poly -> INTT" of CRT polynomials in place:
 * CrtRlwe::mul_dcrt_polynomial_to (primus_lattice/src/rlwe/crt.rs:42-65) followed by
 * DcrtRlwe::into_coeff_form (primus_lattice/src/macros/mod.rs:901-911) per CRT polynomial.
 * Contract (the reference's: reduce_mul_slice_assign takes canonical operands, primus_reduce/src/slice_ops.rs:137-229):
 * crt_poly_dev AND dcrt_poly_dev hold CANONICAL residues in [0, q_i).  A lazily transformed multiplicand ([0, 4q), the
 * output of lazy_transform_slice) is outside the contract: the fused kernels multiply the forward half's unreduced words
 * (up to 2^63 + 3q) by it with one 128 -> 64-bit reduction whose precondition is product < q * 2^64.  Reduce it first
 * (pfhe_dcrt_transform_dev with lazy = 0 gives canonical values). */
int pfhe_dcrt_mul_dcrt_polynomial_dev(const pfhe_dcrt *table, uint64_t *crt_poly_dev,
                                      size_t len, const uint64_t *dcrt_poly_dev, size_t len_b,
                                      void *stream);

/* ---- element-wise family on canonical residues (coefficient or NTT form alike) ----
 * CrtPolynomial / DcrtPolynomial: add, sub, neg (primus_poly/src/{crt,dcrt}/{add,sub,neg}.rs), mul_scalar,
 * add_mul_scalar, mul_factor, add_mul_factor, mul_monomial (crt/mul.rs:16-180, dcrt/mul.rs:78-300), inv
 * (dcrt/inv.rs:19-68); CrtGlwe::{add,sub}_element_wise{,_assign,_to} (primus_lattice/src/macros/mod.rs:367-531),
 * CrtGlwe::mul_scalar_{assign,to}, mul_factor_to, mul_monic_monomial_assign (glwe/crt.rs:59-175) — a GLWE is k+1
 * consecutive RNS polynomials, so the same entry points serve both.
 * `len` = total words, a multiple of L*N; every buffer holds `len` words; `out` may alias `a` (the *_assign
 * forms) and, for sub, `b` (sub_rev_assign, crt/sub.rs:69).  Inputs must be canonical ([0, q_r)), as in the
 * reference.  `scalars`: L residues on the host; `factors`: L ShoupFactor (value, quotient) pairs on the host.
 * The single-modulus NttPolynomial / Polynomial forms (primus_poly/src/ntt/{add,sub,neg,inv}.rs) are the L = 1 case:
 * bind them to a pfhe_dcrt created with one modulus.  add / sub / neg / mul_monomial / inv take tables of any number
 * of limbs; the forms with per-limb scalars or factors up to 32 (UNSUPPORTED beyond). */
int pfhe_dcrt_add_to_dev(const pfhe_dcrt *table, const uint64_t *a_dev, const uint64_t *b_dev, uint64_t *out_dev,
                         size_t len, void *stream);
int pfhe_dcrt_sub_to_dev(const pfhe_dcrt *table, const uint64_t *a_dev, const uint64_t *b_dev, uint64_t *out_dev,
                         size_t len, void *stream);
int pfhe_dcrt_neg_to_dev(const pfhe_dcrt *table, const uint64_t *a_dev, uint64_t *out_dev, size_t len, void *stream);
int pfhe_dcrt_mul_scalar_to_dev(const pfhe_dcrt *table, const uint64_t *a_dev, const uint64_t *scalars,
                                uint64_t *out_dev, size_t len, void *stream);
int pfhe_dcrt_add_mul_scalar_assign_dev(const pfhe_dcrt *table, uint64_t *acc_dev, const uint64_t *rhs_dev,
                                        const uint64_t *scalars, size_t len, void *stream);
int pfhe_dcrt_mul_factor_to_dev(const pfhe_dcrt *table, const uint64_t *a_dev, const uint64_t *factors,
                                uint64_t *out_dev, size_t len, void *stream);
int pfhe_dcrt_add_mul_factor_assign_dev(const pfhe_dcrt *table, uint64_t *acc_dev, const uint64_t *rhs_dev,
                                        const uint64_t *factors, size_t len, void *stream);
/* self * X^r, 0 <= r < 2N, per N-word polynomial (rotate_right + negation of the wrapped part).  The _to form
 * needs out != a and moves each word once; the in-place form keeps a polynomial in one workgroup's registers for
 * 2^9 <= N <= 2^14 and goes through a stream-ordered scratch tile (twice the traffic, not capturable) otherwise. */
int pfhe_dcrt_mul_monomial_to_dev(const pfhe_dcrt *table, const uint64_t *a_dev, size_t r, uint64_t *out_dev,
                                  size_t len, void *stream);
int pfhe_dcrt_mul_monomial_assign_dev(const pfhe_dcrt *table, uint64_t *data_dev, size_t r, size_t len, void *stream);
/* CrtGlwe::mul_monic_monomial_assign (glwe/crt.rs:76-114) with one exponent per element: element e (polys_per_exp
 * RNS polynomials, polys_per_exp x L x N words) of a_dev is multiplied by X^{exps_dev[e]} into out_dev.  Each exponent is
 * taken modulo 2N (read on the device only, never by the host); len must be a whole number of elements; out_dev must not
 * overlap a_dev.  exps_dev holds len / (polys_per_exp * L * N) uint32 exponents.  (The X^{-b_e} * TV of a bootstrap.) */
int pfhe_dcrt_mul_monomial_each_to_dev(const pfhe_dcrt *table, const uint64_t *a_dev, size_t len, const uint32_t *exps_dev,
                                       size_t polys_per_exp, uint64_t *out_dev, void *stream);
/* Point-wise inverse.  The reference panics on a non-invertible element; this call synchronises the stream and
 * returns PFHE_ERR_NO_INVERSE (outputs unspecified).  Not capturable into a HIP graph. */
int pfhe_dcrt_inv_to_dev(const pfhe_dcrt *table, const uint64_t *a_dev, uint64_t *out_dev, size_t len, void *stream);

/* =====================================================================================
 * RNSBase<u64, BarrettModulus<u64>> — primus_rns/src/base.rs:26
 * ===================================================================================== */
typedef struct pfhe_rns pfhe_rns;

/* RNSBase::new(moduli) — base.rs:79-117.  Errors: EMPTY_BASE (:47-49), COPRIME (:83-89),
 * UNREPRESENTABLE_MODULUS when a modulus is not in (1, 2^62) (BarrettModulus::new,
 * primus_modulus/src/barrett/mod.rs:39-44), UNSUPPORTED for more than 32 moduli (bases of up to 8 moduli carry their
 * constants as kernel arguments, wider ones — up to 32 — in a device table owned by the handle and shared with the
 * bases, converters and plans derived from it; the same limit holds for both bases of a pfhe_conv). */
int pfhe_rns_create(const uint64_t *moduli, size_t count, int device, pfhe_rns **out);
void pfhe_rns_destroy(pfhe_rns *base);
size_t pfhe_rns_moduli_count(const pfhe_rns *base);        /* base.rs:124 */
size_t pfhe_rns_big_uint_value_len(const pfhe_rns *base);  /* base.rs:139 */
int pfhe_rns_moduli_product(const pfhe_rns *base, uint64_t *out, size_t len); /* base.rs:133 */
/* compose_multiple_values_to — base.rs:648-675 (-> compose_to :609-633): residue i of value c is
 * multi_residues[i*value_count + c] (modulus-major); value c is written as big_uint_value_len
 * little-endian limbs at big_uint_values[c*big_uint_value_len], canonical in [0, Q). */
int pfhe_rns_compose_multiple_values_to(const pfhe_rns *base, const uint64_t *multi_residues,
                                        size_t len_in, uint64_t *big_uint_values, size_t len_out,
                                        size_t value_count);
int pfhe_rns_compose_multiple_values_to_dev(const pfhe_rns *base, const uint64_t *multi_residues_dev,
                                            size_t len_in, uint64_t *big_uint_values_dev,
                                            size_t len_out, size_t value_count, void *stream);
/* wrapping_decompose_small_values_to — base.rs:279-312 (+ :721-730): centred lift of u in
 * [0, small_value_modulus): u < ceil(m/2) ? u : q_i - m + u ; m == 2 copies. */
int pfhe_rns_wrapping_decompose_small_values_to(const pfhe_rns *base, const uint64_t *small_values,
                                                size_t value_count, uint64_t *multi_residues,
                                                size_t len_out, uint64_t small_value_modulus);
int pfhe_rns_wrapping_decompose_small_values_to_dev(const pfhe_rns *base,
                                                    const uint64_t *small_values_dev,
                                                    size_t value_count, uint64_t *multi_residues_dev,
                                                    size_t len_out, uint64_t small_value_modulus,
                                                    void *stream);
/* add_wrapping_decompose_small_values_scaled — base.rs:326-384 (+ slice::wrapping_decompose_chunk_scaled_to
 * :739-757): acc[i][c] = reduce_add(acc[i][c], factor_i * lift_i(small[c])) with the centred lift above (m == 2
 * takes the unsigned branch, base.rs:371-378); add_decompose_small_values_scaled — base.rs:398-416: the same
 * without the lift (= add_decompose_small_polynomial_scaled, :429-443).  `acc`: L*value_count words,
 * modulus-major, accumulated in place; `factors`: L ShoupFactor (value, quotient) pairs on the host. */
int pfhe_rns_add_wrapping_decompose_small_values_scaled(const pfhe_rns *base, const uint64_t *small_values,
                                                        size_t value_count, uint64_t *acc, size_t len_acc,
                                                        uint64_t small_value_modulus, const uint64_t *factors);
int pfhe_rns_add_wrapping_decompose_small_values_scaled_dev(const pfhe_rns *base, const uint64_t *small_values_dev,
                                                            size_t value_count, uint64_t *acc_dev, size_t len_acc,
                                                            uint64_t small_value_modulus, const uint64_t *factors,
                                                            void *stream);
int pfhe_rns_add_decompose_small_values_scaled(const pfhe_rns *base, const uint64_t *small_values, size_t value_count,
                                               uint64_t *acc, size_t len_acc, const uint64_t *factors);
int pfhe_rns_add_decompose_small_values_scaled_dev(const pfhe_rns *base, const uint64_t *small_values_dev,
                                                   size_t value_count, uint64_t *acc_dev, size_t len_acc,
                                                   const uint64_t *factors, void *stream);

/* =====================================================================================
 * BigUintApproxSignedBasis<u64> — primus_decompose/src/big_integer/basis.rs:17
 * ===================================================================================== */
typedef struct pfhe_basis pfhe_basis;

/* BigUintApproxSignedBasis::new(Q, log_basis, reverse_length, rns_base) — basis.rs:40-211.
 * reverse_length == 0 means None (full chain).  The reference asserts; we return BAD_ARGUMENT. */
int pfhe_basis_create(const pfhe_rns *base, uint32_t log_basis, size_t reverse_length,
                      pfhe_basis **out);
void pfhe_basis_destroy(pfhe_basis *basis);
size_t pfhe_basis_decompose_length(const pfhe_basis *basis); /* basis.rs:236 */
uint32_t pfhe_basis_log_basis(const pfhe_basis *basis);      /* :242 */
uint32_t pfhe_basis_drop_bits(const pfhe_basis *basis);      /* :248 */
uint64_t pfhe_basis_basis_value(const pfhe_basis *basis);    /* :224 */
/* scalar_iter (:283) = 2^(drop + j*log_basis) as big_uint_value_len limbs per level;
 * iter_scalar_residues (:266) = the same reduced modulo every RNS modulus. */
int pfhe_basis_scalars(const pfhe_basis *basis, uint64_t *out, size_t len);
int pfhe_basis_scalars_residue(const pfhe_basis *basis, uint64_t *out, size_t len);
/* init_value_carry_slice_inplace — basis.rs:326-367.  carries are one byte (0/1) per value. */
int pfhe_basis_init_value_carry_slice_inplace(const pfhe_basis *basis, uint64_t *values, size_t len,
                                              uint8_t *carries, size_t count);
int pfhe_basis_init_value_carry_slice_inplace_dev(const pfhe_basis *basis, uint64_t *values_dev,
                                                  size_t len, uint8_t *carries_dev, size_t count,
                                                  void *stream);
/* decomposer_iter().nth(level).unsigned_decompose_slice_to — big_integer/common.rs:309-325
 * (-> unsigned_decompose_to :275-285); level 0 is the least significant digit. */
int pfhe_basis_unsigned_decompose_slice_to(const pfhe_basis *basis, size_t level,
                                           const uint64_t *values, size_t len, uint64_t *digits,
                                           uint8_t *carries, size_t count);
int pfhe_basis_unsigned_decompose_slice_to_dev(const pfhe_basis *basis, size_t level,
                                               const uint64_t *values_dev, size_t len,
                                               uint64_t *digits_dev, uint8_t *carries_dev,
                                               size_t count, void *stream);
/* init_value_carry_slice_to — basis.rs:371-420: the out-of-place form (input untouched). */
int pfhe_basis_init_value_carry_slice_to(const pfhe_basis *basis, const uint64_t *values, size_t len,
                                         uint64_t *adjusted_values, uint8_t *carries, size_t count);
int pfhe_basis_init_value_carry_slice_to_dev(const pfhe_basis *basis, const uint64_t *values_dev, size_t len,
                                             uint64_t *adjusted_values_dev, uint8_t *carries_dev, size_t count,
                                             void *stream);
/* decomposer_iter().nth(level).decompose_slice_to — big_integer/common.rs:289-306 (-> decompose_to :255-272): the
 * SIGNED digit as a residue modulo Q, big_uint_value_len limbs per value (a negative digit d is stored as Q + d);
 * len_out must equal len; input and output must be distinct buffers. */
int pfhe_basis_decompose_slice_to(const pfhe_basis *basis, size_t level, const uint64_t *values, size_t len,
                                  uint64_t *decomposed_values, size_t len_out, uint8_t *carries, size_t count);
int pfhe_basis_decompose_slice_to_dev(const pfhe_basis *basis, size_t level, const uint64_t *values_dev, size_t len,
                                      uint64_t *decomposed_values_dev, size_t len_out, uint8_t *carries_dev,
                                      size_t count, void *stream);

/* =====================================================================================
 * RNS gadget external product — primus_lattice
 * ===================================================================================== */
typedef struct pfhe_extprod_plan pfhe_extprod_plan;

/* Bundles what the reference passes as (&BigUintApproxSignedBasis, &Table, &RNSBase,
 * &mut DcrtGlevContext) — glwe/crt.rs:200-212, context/glev.rs:4-68.  The plan borrows `table`
 * (which must outlive it) and owns device scratch for `chunk` ciphertexts (0 = default: about 1 GiB of digit polynomials
 * per buffer, at least 64 and at most 65536 ciphertexts):
 * one buffer of chunk*(k+1)*ell*L*N words (+ chunk*(k+1)*ell*N balanced digits: int32 for log_basis <= 31, else int64).
 * Like `&mut DcrtGlevContext` (context/glev.rs:4-10) the plan has ONE holder at a time, and that is enforced: every
 * pfhe_extprod_* call takes the plan for its duration, and a call from a second thread meanwhile returns
 * PFHE_ERR_BUSY ("plan in use") instead of racing on the digit buffers (pfhe_extprod_plan_in_use reports the
 * flag; one plan per thread).  Streams: device-pointer calls return when their kernels are queued; the plan remembers an event
 * behind its last call and a call on a DIFFERENT stream first makes that stream wait for it, so using one plan from one
 * stream after another needs no event handling by the caller (round 5; until then this was the caller's job).  Work
 * captured into a HIP graph is outside that bookkeeping: do not replay a graph that uses a plan beside other users of it. */
int pfhe_extprod_plan_create(const pfhe_dcrt *table, const pfhe_rns *base, const pfhe_basis *basis,
                             size_t glwe_dimension, size_t chunk, pfhe_extprod_plan **out);
void pfhe_extprod_plan_destroy(pfhe_extprod_plan *plan);
int pfhe_extprod_plan_in_use(const pfhe_extprod_plan *plan);  /* 1 while some thread is inside a pfhe_extprod_* call on it */
/* Test aid, not a reference interface: hold != 0 takes the plan for the calling thread exactly as an entry point does
 * (PFHE_ERR_BUSY when another thread holds it) and keeps it until the same thread calls with hold == 0. */
int pfhe_extprod_plan_debug_hold(pfhe_extprod_plan *plan, int hold);
size_t pfhe_extprod_plan_scratch_bytes(const pfhe_extprod_plan *plan);
/* CrtGlwe::mul_dcrt_ggsw_to — glwe/crt.rs:200-227.  crt_glwe: batch x (k+1) CRT polynomials
 * |a1|..|ak|b|; dcrt_ggsw: ONE GGSW shared by the batch or batch GGSWs, each
 * (k+1) rows x ell levels x (k+1) components x L x N words; result: batch DcrtGlwe (NTT form), or
 * coefficient form when into_coeff_form != 0 (DcrtGlwe::into_coeff_form, macros/mod.rs:901-911). */
int pfhe_extprod_mul_dcrt_ggsw_to(pfhe_extprod_plan *plan, const uint64_t *crt_glwe, size_t len_glwe,
                                  const uint64_t *dcrt_ggsw, size_t len_ggsw, uint64_t *result,
                                  size_t len_result, int into_coeff_form);
int pfhe_extprod_mul_dcrt_ggsw_to_dev(pfhe_extprod_plan *plan, const uint64_t *crt_glwe_dev,
                                      size_t len_glwe, const uint64_t *dcrt_ggsw_dev, size_t len_ggsw,
                                      uint64_t *result_dev, size_t len_result, int into_coeff_form,
                                      void *stream);
/* Measurement aid (bench.py, tools/): the same product (coefficient-form output) with HIP events between its kernel
 * groups on `stream`; waits for the stream.  ms_out[0] = digit extraction + lifting strided pass, ms_out[1] = block pass of
 * the digits' transform + multiply-accumulate (+ the inverse transform's block pass, fused into the same kernel), both
 * summed over the *launches_out chunks; the inverse transform's strided pass runs after the last event.  Not a reference
 * interface. */
int pfhe_extprod_profile_dev(pfhe_extprod_plan *plan, const uint64_t *crt_glwe_dev, size_t len_glwe,
                             const uint64_t *dcrt_ggsw_dev, size_t len_ggsw, uint64_t *result_dev, size_t len_result,
                             double *ms_out, size_t *launches_out, void *stream);
/* DcrtGlwe::add_dcrt_glev_mul_crt_poly_assign — glwe/dcrt.rs:178-255: acc += glev (x) crt_poly. */
int pfhe_extprod_add_dcrt_glev_mul_crt_poly_assign_dev(pfhe_extprod_plan *plan, uint64_t *acc_dev,
                                                       size_t len_acc, const uint64_t *dcrt_glev_dev,
                                                       size_t len_glev, const uint64_t *crt_poly_dev,
                                                       size_t len_poly, void *stream);

/* DcrtGlev::mul_crt_poly_to — primus_lattice/src/glev/dcrt.rs:45-110: result = glev (x) crt_poly
 * (one GGSW row; overwrites instead of accumulating). */
int pfhe_extprod_glev_mul_crt_poly_to_dev(pfhe_extprod_plan *plan, const uint64_t *dcrt_glev_dev,
                                          size_t len_glev, const uint64_t *crt_poly_dev, size_t len_poly,
                                          uint64_t *result_dev, size_t len_result, void *stream);
/* The same two products with the polynomial given as a BigUintPolynomial (big_uint_value_len limbs per
 * coefficient, canonical modulo Q): DcrtGlwe::add_dcrt_glev_mul_big_uint_poly_assign — glwe/dcrt.rs:258-338 — and
 * DcrtGlev::mul_big_uint_poly_to — glev/dcrt.rs:113-175.  len_poly = batch * big_uint_value_len * N. */
int pfhe_extprod_add_dcrt_glev_mul_big_uint_poly_assign_dev(pfhe_extprod_plan *plan, uint64_t *acc_dev, size_t len_acc,
                                                            const uint64_t *dcrt_glev_dev, size_t len_glev,
                                                            const uint64_t *big_uint_poly_dev, size_t len_poly,
                                                            void *stream);
int pfhe_extprod_glev_mul_big_uint_poly_to_dev(pfhe_extprod_plan *plan, const uint64_t *dcrt_glev_dev, size_t len_glev,
                                               const uint64_t *big_uint_poly_dev, size_t len_poly, uint64_t *result_dev,
                                               size_t len_result, void *stream);

/* =====================================================================================
 * Batched blind rotation over the external product — the CMUX loop of a bootstrap
 * ===================================================================================== */
typedef struct pfhe_blindrot pfhe_blindrot;

/* For every step i = 0 .. n_steps-1 in order, and every ciphertext e of the batch:
 *   D     = X^{exps[e*n_steps+i]} * ACC_e - ACC_e    CrtGlwe::mul_monic_monomial_assign (glwe/crt.rs:76-114),
 *                                                    sub_element_wise_assign (macros/mod.rs:438)
 *   E     = coeff_form(D (x) BSK_i)                  CrtGlwe::mul_dcrt_ggsw_to (glwe/crt.rs:200-227),
 *                                                    DcrtGlwe::write_coeff_form (macros/mod.rs:921)
 *   ACC_e = ACC_e + E                                add_element_wise_assign (macros/mod.rs:410)
 * acc: batch CrtGlwe in coefficient form ((k+1) x L x N words each), read and written in place; bsk: n_steps DcrtGgsw end
 * to end ((k+1) x ell x (k+1) x L x N words each), shared by the batch; exps: batch x n_steps uint32, ciphertext-major.
 * batch = len_acc / ((k+1)*L*N), n_steps = len_bsk / ggsw words; PFHE_ERR_BAD_LENGTH unless both divide evenly and
 * len_exps == batch * n_steps; n_steps == 0 is a no-op.  Output canonical, bit-identical to that sequence.
 * The handle borrows `table` (which must outlive it) and owns an external-product plan (pfhe_extprod_plan_create with the
 * same arguments) plus three glue buffers of chunk ciphertexts, all allocated here; a batch larger than the chunk runs
 * chunk by chunk, every step of a chunk before the next chunk.  One holder at a time, as the plan (PFHE_ERR_BUSY).
 * N = 2^10 / 2^11 with k = 1 (where the external product takes its small-ring kernel: at least 1024 (ciphertext, limb)
 * pairs per chunk, fused kernels enabled when the handle was created) runs two launches per step; every other shape runs
 * the product and one glue launch per step. */
int pfhe_blindrot_create(const pfhe_dcrt *table, const pfhe_rns *base, const pfhe_basis *basis, size_t glwe_dimension,
                         size_t chunk, pfhe_blindrot **out);
void pfhe_blindrot_destroy(pfhe_blindrot *h);
int pfhe_blindrot_in_use(const pfhe_blindrot *h);  /* 1 while some thread is inside a pfhe_blindrot_* call on it */
size_t pfhe_blindrot_scratch_bytes(const pfhe_blindrot *h);
/* Device form: every exponent is taken modulo 2N on the device.  All work is queued on `stream`, with no host
 * synchronisation and no allocation, so a whole rotation can be captured into a HIP graph. */
int pfhe_blindrot_rotate_dev(pfhe_blindrot *h, uint64_t *acc_dev, size_t len_acc, const uint64_t *bsk_dev, size_t len_bsk,
                             const uint32_t *exps_dev, size_t len_exps, void *stream);
/* Host form: PFHE_ERR_BAD_ARGUMENT for any exponent of 2N or more (the reference's debug_assert!(r < 2N)). */
int pfhe_blindrot_rotate(pfhe_blindrot *h, uint64_t *acc, size_t len_acc, const uint64_t *bsk, size_t len_bsk,
                         const uint32_t *exps, size_t len_exps);

/* Profiling hooks (bench.py / rocprofv3): a transform is executed as a short sequence of kernel
 * passes (DESIGN.md "Kernels"); these run or name ONE pass so that each kernel can be timed with
 * HIP events in isolation.  The data is only meaningful after all passes have run in order. */
int pfhe_dcrt_transform_num_passes(const pfhe_dcrt *table);
const char *pfhe_dcrt_transform_pass_name(const pfhe_dcrt *table, int inverse, int index);
int pfhe_dcrt_transform_pass_dev(const pfhe_dcrt *table, uint64_t *poly_dev, size_t len, int inverse,
                                 int index, int lazy, void *stream);
/* How pfhe_dcrt_transform_dev / pfhe_dcrt_inverse_transform_dev will run `len` words: the kernel (or form) name and
 * the number of kernel launches.  Large batches of N = 2^16 run as tiles + 1 launches of ntt_pipe_{fwd,inv}_kernel (block pass of
 * one tile and strided pass of the next in each workgroup), not as the per-pass kernels above. */
int pfhe_dcrt_transform_form(const pfhe_dcrt *table, size_t len, int inverse, char *name, size_t cap,
                             int *launches);

/* =====================================================================================
 * BaseConverter — primus_rns/src/converter.rs:21 — and RNSBase::decompose_big_uint_values_to
 * (primus_rns/src/base.rs:457-481).  Residue arrays are modulus-major, as in the reference; the
 * reference's coefficient-major `scratch` argument has no counterpart (the scaled residues stay
 * in registers).
 * ===================================================================================== */
typedef struct pfhe_conv pfhe_conv;

/* BaseConverter::new(input_base, output_base) — converter.rs:43-69 (the bases are copied) */
int pfhe_conv_create(const pfhe_rns *input_base, const pfhe_rns *output_base, pfhe_conv **out);
void pfhe_conv_destroy(pfhe_conv *conv);
size_t pfhe_conv_input_moduli_count(const pfhe_conv *conv);  /* converter.rs:82 */
size_t pfhe_conv_output_moduli_count(const pfhe_conv *conv); /* :87 */
/* row-major output-by-input matrix (Q/q_i) mod p_j — converter.rs:28-32 */
int pfhe_conv_base_change_matrix(const pfhe_conv *conv, uint64_t *out, size_t len);
/* fast_convert_array — converter.rs:192-218.  len_in = L_in * poly_length, len_out = L_out *
 * poly_length. */
int pfhe_conv_fast_convert_array(const pfhe_conv *conv, const uint64_t *crt_poly_in, size_t len_in,
                                 uint64_t *crt_poly_out, size_t len_out, size_t poly_length);
int pfhe_conv_fast_convert_array_dev(const pfhe_conv *conv, const uint64_t *crt_poly_in_dev,
                                     size_t len_in, uint64_t *crt_poly_out_dev, size_t len_out,
                                     size_t poly_length, void *stream);
/* fast_convert_array_to_pair_iter — converter.rs:233-272: two output moduli; `pairs_out_dev`
 * receives poly_length interleaved (mod p_0, mod p_1) pairs (len_out = 2 * poly_length) */
int pfhe_conv_fast_convert_array_to_pairs_dev(const pfhe_conv *conv, const uint64_t *crt_poly_in_dev,
                                              size_t len_in, uint64_t *pairs_out_dev,
                                              size_t len_out, size_t poly_length, void *stream);
/* exact_convert_array — converter.rs:274-364 (single output modulus; f64 correction term) */
int pfhe_conv_exact_convert_array(const pfhe_conv *conv, const uint64_t *crt_poly_in, size_t len_in,
                                  uint64_t *crt_poly_out, size_t len_out, size_t poly_length);
int pfhe_conv_exact_convert_array_dev(const pfhe_conv *conv, const uint64_t *crt_poly_in_dev,
                                      size_t len_in, uint64_t *crt_poly_out_dev, size_t len_out,
                                      size_t poly_length, void *stream);
/* RNSBase::decompose_big_uint_values_to — base.rs:457-481 */
int pfhe_rns_decompose_big_uint_values_to(const pfhe_rns *base, const uint64_t *big_uint_values,
                                          size_t len_in, uint64_t *multi_residues, size_t len_out,
                                          size_t value_count);
int pfhe_rns_decompose_big_uint_values_to_dev(const pfhe_rns *base,
                                              const uint64_t *big_uint_values_dev, size_t len_in,
                                              uint64_t *multi_residues_dev, size_t len_out,
                                              size_t value_count, void *stream);

/* =====================================================================================
 * u32 tables — U32NttTable (primus_ntt/src/ntt/prime32/table.rs:37-91, NttTable impl :184-470)
 * and U32DcrtTable (primus_ntt/src/dcrt/prime32.rs:11-128).  Same contracts as the 64-bit
 * tables with uint32_t words; q < 2^30 (table.rs:195-200 -> PFHE_ERR_MODULUS_TOO_LARGE).
 * Butterflies are the reference's Barrett-32 ones (prime32/scalar/arithmetic.rs:16-51).
 * ===================================================================================== */
typedef struct pfhe_ntt32 pfhe_ntt32;

/* NttTable::new — prime32/table.rs:184-333 */
int pfhe_ntt32_create(uint32_t log_n, uint32_t modulus, int device, pfhe_ntt32 **out);
void pfhe_ntt32_destroy(pfhe_ntt32 *table);
/* getters — table.rs:103-137 */
size_t pfhe_ntt32_poly_length(const pfhe_ntt32 *table);
uint32_t pfhe_ntt32_log_n(const pfhe_ntt32 *table);
uint32_t pfhe_ntt32_modulus(const pfhe_ntt32 *table);
uint32_t pfhe_ntt32_root(const pfhe_ntt32 *table);
uint32_t pfhe_ntt32_inv_root(const pfhe_ntt32 *table);
uint32_t pfhe_ntt32_inv_n(const pfhe_ntt32 *table);
int pfhe_ntt32_device(const pfhe_ntt32 *table);
/* transform_slice / inverse_transform_slice / lazy_* — table.rs:356-374 (host pointers) */
int pfhe_ntt32_transform_slice(const pfhe_ntt32 *table, uint32_t *poly, size_t len);
int pfhe_ntt32_inverse_transform_slice(const pfhe_ntt32 *table, uint32_t *values, size_t len);
int pfhe_ntt32_lazy_transform_slice(const pfhe_ntt32 *table, uint32_t *poly, size_t len);
int pfhe_ntt32_lazy_inverse_transform_slice(const pfhe_ntt32 *table, uint32_t *values, size_t len);
/* transform_monomial / transform_coeff_one_monomial / transform_coeff_minus_one_monomial —
 * table.rs:376-470 */
int pfhe_ntt32_transform_monomial(const pfhe_ntt32 *table, uint32_t coeff, size_t degree,
                                  uint32_t *values, size_t len);
int pfhe_ntt32_transform_coeff_one_monomial(const pfhe_ntt32 *table, size_t degree,
                                            uint32_t *values, size_t len);
int pfhe_ntt32_transform_coeff_minus_one_monomial(const pfhe_ntt32 *table, size_t degree,
                                                  uint32_t *values, size_t len);
/* device-pointer variants */
int pfhe_ntt32_transform_dev(const pfhe_ntt32 *table, uint32_t *poly_dev, size_t len, int lazy,
                             void *stream);
int pfhe_ntt32_inverse_transform_dev(const pfhe_ntt32 *table, uint32_t *values_dev, size_t len,
                                     int lazy, void *stream);
int pfhe_ntt32_transform_monomial_dev(const pfhe_ntt32 *table, uint32_t coeff, size_t degree,
                                      uint32_t *values_dev, size_t len, void *stream);
/* NttPolynomial<u32>::mul_assign / add_mul_assign (primus_poly/src/ntt/mul.rs:84-90,
 * ntt/mod.rs:101-112 with BarrettModulus<u32>) */
int pfhe_ntt32_mul_assign_dev(const pfhe_ntt32 *table, uint32_t *a_dev, size_t len_a,
                              const uint32_t *b_dev, size_t len_b, void *stream);
int pfhe_ntt32_add_mul_assign_dev(const pfhe_ntt32 *table, uint32_t *acc_dev,
                                  const uint32_t *a_dev, size_t len_a, const uint32_t *b_dev,
                                  size_t len_b, void *stream);

typedef struct pfhe_dcrt32 pfhe_dcrt32;

/* DcrtTable::new — dcrt/prime32.rs:24-43 */
int pfhe_dcrt32_create(uint32_t log_n, const uint32_t *moduli, size_t moduli_count, int device,
                       pfhe_dcrt32 **out);
void pfhe_dcrt32_destroy(pfhe_dcrt32 *table);
size_t pfhe_dcrt32_poly_length(const pfhe_dcrt32 *table);     /* dcrt/prime32.rs:56 */
size_t pfhe_dcrt32_moduli_count(const pfhe_dcrt32 *table);    /* :61 */
size_t pfhe_dcrt32_crt_poly_length(const pfhe_dcrt32 *table); /* :66 */
int pfhe_dcrt32_device(const pfhe_dcrt32 *table);
uint32_t pfhe_dcrt32_modulus(const pfhe_dcrt32 *table, size_t i);
uint32_t pfhe_dcrt32_root(const pfhe_dcrt32 *table, size_t i);
/* transform_slice / inverse_transform_slice / lazy_* — dcrt/prime32.rs:96-127 */
int pfhe_dcrt32_transform_slice(const pfhe_dcrt32 *table, uint32_t *poly, size_t len);
int pfhe_dcrt32_inverse_transform_slice(const pfhe_dcrt32 *table, uint32_t *poly, size_t len);
int pfhe_dcrt32_lazy_transform_slice(const pfhe_dcrt32 *table, uint32_t *poly, size_t len);
int pfhe_dcrt32_lazy_inverse_transform_slice(const pfhe_dcrt32 *table, uint32_t *poly, size_t len);
/* DcrtTable::transform_monomial & co — dcrt/mod.rs:107-134 */
int pfhe_dcrt32_transform_monomial(const pfhe_dcrt32 *table, uint32_t coeff, size_t degree,
                                   uint32_t *values, size_t len);
int pfhe_dcrt32_transform_coeff_one_monomial(const pfhe_dcrt32 *table, size_t degree,
                                             uint32_t *values, size_t len);
int pfhe_dcrt32_transform_coeff_minus_one_monomial(const pfhe_dcrt32 *table, size_t degree,
                                                   uint32_t *values, size_t len);
int pfhe_dcrt32_transform_dev(const pfhe_dcrt32 *table, uint32_t *poly_dev, size_t len, int lazy,
                              void *stream);
int pfhe_dcrt32_inverse_transform_dev(const pfhe_dcrt32 *table, uint32_t *poly_dev, size_t len,
                                      int lazy, void *stream);
/* DcrtPolynomial<u32>::mul_assign / add_mul_assign — primus_poly/src/dcrt/mul.rs:176-187,
 * dcrt/mod.rs:105-123 */
int pfhe_dcrt32_mul_assign_dev(const pfhe_dcrt32 *table, uint32_t *a_dev, size_t len_a,
                               const uint32_t *b_dev, size_t len_b, void *stream);
int pfhe_dcrt32_add_mul_assign_dev(const pfhe_dcrt32 *table, uint32_t *acc_dev,
                                   const uint32_t *a_dev, size_t len_a, const uint32_t *b_dev,
                                   size_t len_b, void *stream);
/* synthetic residues: word i = floor(splitmix64(seed, i) * q_limb(i) / 2^64) */
int pfhe_dcrt32_fill_uniform_dev(const pfhe_dcrt32 *table, uint32_t *dst_dev, size_t len,
                                 uint64_t seed, void *stream);
/* profiling hooks (one kernel launch per pass), as pfhe_dcrt_transform_pass_dev */
int pfhe_dcrt32_transform_num_passes(const pfhe_dcrt32 *table);
const char *pfhe_dcrt32_transform_pass_name(const pfhe_dcrt32 *table, int inverse, int index);
/* as pfhe_dcrt_transform_form: the kernel (or form) a transform of `len` words runs as, and its number of launches */
int pfhe_dcrt32_transform_form(const pfhe_dcrt32 *table, size_t len, int inverse, char *name, size_t cap, int *launches);
int pfhe_dcrt32_transform_pass_dev(const pfhe_dcrt32 *table, uint32_t *poly_dev, size_t len,
                                   int inverse, int index, int lazy, void *stream);

/* =====================================================================================
 * The <u32> instantiations of the same generics: RNSBase<u32, BarrettModulus<u32>> (primus_rns/src/base.rs:26-37),
 * BigUintApproxSignedBasis<u32> (primus_decompose/src/big_integer/basis.rs:33 — the type the reference's own
 * tests/big_uint.rs:13 runs) and CrtGlwe<u32>::mul_dcrt_ggsw_to over a U32DcrtTable (primus_lattice/src/glwe/crt.rs:200-227,
 * primus_ntt/src/dcrt/prime32.rs:11).  Same contracts as the 64-bit entry points above with uint32_t words: residues,
 * digits and the limbs of big integers are u32 in memory (big_uint_value_len counts u32 limbs: as many as Q needs,
 * big_integer.rs:675-686); moduli below 2^30; log_basis below 32.  Every output is the canonical integer the reference's
 * u32 arithmetic produces.
 * ===================================================================================== */
typedef struct pfhe_rns32 pfhe_rns32;
typedef struct pfhe_basis32 pfhe_basis32;
typedef struct pfhe_extprod32_plan pfhe_extprod32_plan;
typedef struct pfhe_blindrot32 pfhe_blindrot32;

/* RNSBase::new(moduli) — base.rs:79-117.  Errors: EMPTY_BASE (:47-49), COPRIME (:83-89),
 * UNREPRESENTABLE_MODULUS when a modulus is not in (1, 2^30) (BarrettModulus::<u32>::new,
 * primus_modulus/src/barrett/mod.rs:39-44), UNSUPPORTED for more than 32 moduli (bases of up to 8 moduli carry their
 * constants as kernel arguments, wider ones — up to 32 — in a device table owned by the handle and shared with the
 * bases, converters and plans derived from it; the same limit holds for both bases of a pfhe_conv). */
int pfhe_rns32_create(const uint32_t *moduli, size_t count, int device, pfhe_rns32 **out);
void pfhe_rns32_destroy(pfhe_rns32 *base);
size_t pfhe_rns32_moduli_count(const pfhe_rns32 *base);        /* base.rs:124 */
size_t pfhe_rns32_big_uint_value_len(const pfhe_rns32 *base);  /* base.rs:139 */
int pfhe_rns32_moduli_product(const pfhe_rns32 *base, uint32_t *out, size_t len); /* base.rs:133 */
/* compose_multiple_values_to — base.rs:648-675 (-> compose_to :609-633): residue i of value c is
 * multi_residues[i*value_count + c] (modulus-major); value c is written as big_uint_value_len
 * little-endian limbs at big_uint_values[c*big_uint_value_len], canonical in [0, Q). */
int pfhe_rns32_compose_multiple_values_to(const pfhe_rns32 *base, const uint32_t *multi_residues,
                                        size_t len_in, uint32_t *big_uint_values, size_t len_out,
                                        size_t value_count);
int pfhe_rns32_compose_multiple_values_to_dev(const pfhe_rns32 *base, const uint32_t *multi_residues_dev,
                                            size_t len_in, uint32_t *big_uint_values_dev,
                                            size_t len_out, size_t value_count, void *stream);
/* wrapping_decompose_small_values_to — base.rs:279-312 (+ :721-730): centred lift of u in
 * [0, small_value_modulus): u < ceil(m/2) ? u : q_i - m + u ; m == 2 copies. */
int pfhe_rns32_wrapping_decompose_small_values_to(const pfhe_rns32 *base, const uint32_t *small_values,
                                                size_t value_count, uint32_t *multi_residues,
                                                size_t len_out, uint32_t small_value_modulus);
int pfhe_rns32_wrapping_decompose_small_values_to_dev(const pfhe_rns32 *base,
                                                    const uint32_t *small_values_dev,
                                                    size_t value_count, uint32_t *multi_residues_dev,
                                                    size_t len_out, uint32_t small_value_modulus,
                                                    void *stream);
/* add_wrapping_decompose_small_values_scaled — base.rs:326-384 (+ slice::wrapping_decompose_chunk_scaled_to
 * :739-757): acc[i][c] = reduce_add(acc[i][c], factor_i * lift_i(small[c])) with the centred lift above (m == 2
 * takes the unsigned branch, base.rs:371-378); add_decompose_small_values_scaled — base.rs:398-416: the same
 * without the lift (= add_decompose_small_polynomial_scaled, :429-443).  `acc`: L*value_count words,
 * modulus-major, accumulated in place; `factors`: L ShoupFactor<u32> (value, quotient) pairs on the host (quotient = floor(value * 2^32 / q_i)). */
int pfhe_rns32_add_wrapping_decompose_small_values_scaled(const pfhe_rns32 *base, const uint32_t *small_values,
                                                        size_t value_count, uint32_t *acc, size_t len_acc,
                                                        uint32_t small_value_modulus, const uint32_t *factors);
int pfhe_rns32_add_wrapping_decompose_small_values_scaled_dev(const pfhe_rns32 *base, const uint32_t *small_values_dev,
                                                            size_t value_count, uint32_t *acc_dev, size_t len_acc,
                                                            uint32_t small_value_modulus, const uint32_t *factors,
                                                            void *stream);
int pfhe_rns32_add_decompose_small_values_scaled(const pfhe_rns32 *base, const uint32_t *small_values, size_t value_count,
                                               uint32_t *acc, size_t len_acc, const uint32_t *factors);
int pfhe_rns32_add_decompose_small_values_scaled_dev(const pfhe_rns32 *base, const uint32_t *small_values_dev,
                                                   size_t value_count, uint32_t *acc_dev, size_t len_acc,
                                                   const uint32_t *factors, void *stream);

/* BigUintApproxSignedBasis::new(Q, log_basis, reverse_length, rns_base) — basis.rs:40-211.
 * reverse_length == 0 means None (full chain); 0 < log_basis < 32 (:51).  The reference asserts; we return BAD_ARGUMENT. */
int pfhe_basis32_create(const pfhe_rns32 *base, uint32_t log_basis, size_t reverse_length,
                      pfhe_basis32 **out);
void pfhe_basis32_destroy(pfhe_basis32 *basis);
size_t pfhe_basis32_decompose_length(const pfhe_basis32 *basis); /* basis.rs:236 */
uint32_t pfhe_basis32_log_basis(const pfhe_basis32 *basis);      /* :242 */
uint32_t pfhe_basis32_drop_bits(const pfhe_basis32 *basis);      /* :248 */
uint32_t pfhe_basis32_basis_value(const pfhe_basis32 *basis);    /* :224 */
/* scalar_iter (:283) = 2^(drop + j*log_basis) as big_uint_value_len limbs per level;
 * iter_scalar_residues (:266) = the same reduced modulo every RNS modulus. */
int pfhe_basis32_scalars(const pfhe_basis32 *basis, uint32_t *out, size_t len);
int pfhe_basis32_scalars_residue(const pfhe_basis32 *basis, uint32_t *out, size_t len);
/* init_value_carry_slice_inplace — basis.rs:326-367.  carries are one byte (0/1) per value. */
int pfhe_basis32_init_value_carry_slice_inplace(const pfhe_basis32 *basis, uint32_t *values, size_t len,
                                              uint8_t *carries, size_t count);
int pfhe_basis32_init_value_carry_slice_inplace_dev(const pfhe_basis32 *basis, uint32_t *values_dev,
                                                  size_t len, uint8_t *carries_dev, size_t count,
                                                  void *stream);
/* decomposer_iter().nth(level).unsigned_decompose_slice_to — big_integer/common.rs:309-325
 * (-> unsigned_decompose_to :275-285); level 0 is the least significant digit. */
int pfhe_basis32_unsigned_decompose_slice_to(const pfhe_basis32 *basis, size_t level,
                                           const uint32_t *values, size_t len, uint32_t *digits,
                                           uint8_t *carries, size_t count);
int pfhe_basis32_unsigned_decompose_slice_to_dev(const pfhe_basis32 *basis, size_t level,
                                               const uint32_t *values_dev, size_t len,
                                               uint32_t *digits_dev, uint8_t *carries_dev,
                                               size_t count, void *stream);
/* init_value_carry_slice_to — basis.rs:371-420: the out-of-place form (input untouched). */
int pfhe_basis32_init_value_carry_slice_to(const pfhe_basis32 *basis, const uint32_t *values, size_t len,
                                         uint32_t *adjusted_values, uint8_t *carries, size_t count);
int pfhe_basis32_init_value_carry_slice_to_dev(const pfhe_basis32 *basis, const uint32_t *values_dev, size_t len,
                                             uint32_t *adjusted_values_dev, uint8_t *carries_dev, size_t count,
                                             void *stream);
/* decomposer_iter().nth(level).decompose_slice_to — big_integer/common.rs:289-306 (-> decompose_to :255-272): the
 * SIGNED digit as a residue modulo Q, big_uint_value_len limbs per value (a negative digit d is stored as Q + d);
 * len_out must equal len; input and output must be distinct buffers. */
int pfhe_basis32_decompose_slice_to(const pfhe_basis32 *basis, size_t level, const uint32_t *values, size_t len,
                                  uint32_t *decomposed_values, size_t len_out, uint8_t *carries, size_t count);
int pfhe_basis32_decompose_slice_to_dev(const pfhe_basis32 *basis, size_t level, const uint32_t *values_dev, size_t len,
                                      uint32_t *decomposed_values_dev, size_t len_out, uint8_t *carries_dev,
                                      size_t count, void *stream);
/* RNSBase::decompose_big_uint_values_to — base.rs:457-481 */
int pfhe_rns32_decompose_big_uint_values_to(const pfhe_rns32 *base, const uint32_t *big_uint_values,
                                          size_t len_in, uint32_t *multi_residues, size_t len_out,
                                          size_t value_count);
int pfhe_rns32_decompose_big_uint_values_to_dev(const pfhe_rns32 *base,
                                              const uint32_t *big_uint_values_dev, size_t len_in,
                                              uint32_t *multi_residues_dev, size_t len_out,
                                              size_t value_count, void *stream);

/* BaseConverter<u32> — primus_rns/src/converter.rs:21 (generic over T: FheUint): the contracts of pfhe_conv_* with
 * uint32_t residues.  reduce_dot_product folds a 64-bit accumulator every 16 terms there (common/compact/slice.rs:380-405);
 * the value reduced is the same integer, so every output is the canonical residue the reference produces; the exact form
 * rounds with `(sum + 0.5) as u32`. */
typedef struct pfhe_conv32 pfhe_conv32;
int pfhe_conv32_create(const pfhe_rns32 *input_base, const pfhe_rns32 *output_base, pfhe_conv32 **out);
void pfhe_conv32_destroy(pfhe_conv32 *conv);
size_t pfhe_conv32_input_moduli_count(const pfhe_conv32 *conv);
size_t pfhe_conv32_output_moduli_count(const pfhe_conv32 *conv);
int pfhe_conv32_base_change_matrix(const pfhe_conv32 *conv, uint32_t *out, size_t len);
int pfhe_conv32_fast_convert_array(const pfhe_conv32 *conv, const uint32_t *crt_poly_in, size_t len_in,
                                   uint32_t *crt_poly_out, size_t len_out, size_t poly_length);
int pfhe_conv32_fast_convert_array_dev(const pfhe_conv32 *conv, const uint32_t *crt_poly_in_dev, size_t len_in,
                                       uint32_t *crt_poly_out_dev, size_t len_out, size_t poly_length, void *stream);
int pfhe_conv32_fast_convert_array_to_pairs_dev(const pfhe_conv32 *conv, const uint32_t *crt_poly_in_dev, size_t len_in,
                                                uint32_t *pairs_out_dev, size_t len_out, size_t poly_length, void *stream);
int pfhe_conv32_exact_convert_array(const pfhe_conv32 *conv, const uint32_t *crt_poly_in, size_t len_in,
                                    uint32_t *crt_poly_out, size_t len_out, size_t poly_length);
int pfhe_conv32_exact_convert_array_dev(const pfhe_conv32 *conv, const uint32_t *crt_poly_in_dev, size_t len_in,
                                        uint32_t *crt_poly_out_dev, size_t len_out, size_t poly_length, void *stream);

/* The plan of the u32 product: as pfhe_extprod_plan_create (one holder at a time, `table` borrowed, device scratch for
 * `chunk` ciphertexts: chunk*(k+1)*ell*L*N u32 words; 0 = about 1 GiB, at least 128 ciphertexts). */
int pfhe_extprod32_plan_create(const pfhe_dcrt32 *table, const pfhe_rns32 *base, const pfhe_basis32 *basis,
                               size_t glwe_dimension, size_t chunk, pfhe_extprod32_plan **out);
void pfhe_extprod32_plan_destroy(pfhe_extprod32_plan *plan);
int pfhe_extprod32_plan_in_use(const pfhe_extprod32_plan *plan);
size_t pfhe_extprod32_plan_scratch_bytes(const pfhe_extprod32_plan *plan);
/* Precondition of every pfhe_extprod32_* product below: all u32 operands are CANONICAL — each word of the GLWE / CRT
 * polynomials, of the GGSW / GLev key and of an accumulator that a call adds to is below its modulus q_i (< 2^30).  The
 * kernels sum products of such words lazily in 64 bits and fold once per fifteen terms: fifteen products below 2^60 on a
 * folded value stay below 2^64 with nothing to spare, so a word of q_i or more can wrap the sum silently (the reference
 * reduces after every term and would not).  Nothing checks this on the way in. */
/* CrtGlwe::mul_dcrt_ggsw_to — glwe/crt.rs:200-227 (layouts as pfhe_extprod_mul_dcrt_ggsw_to) */
int pfhe_extprod32_mul_dcrt_ggsw_to(pfhe_extprod32_plan *plan, const uint32_t *crt_glwe, size_t len_glwe,
                                    const uint32_t *dcrt_ggsw, size_t len_ggsw, uint32_t *result, size_t len_result,
                                    int into_coeff_form);
int pfhe_extprod32_mul_dcrt_ggsw_to_dev(pfhe_extprod32_plan *plan, const uint32_t *crt_glwe_dev, size_t len_glwe,
                                        const uint32_t *dcrt_ggsw_dev, size_t len_ggsw, uint32_t *result_dev,
                                        size_t len_result, int into_coeff_form, void *stream);
/* DcrtGlwe::add_dcrt_glev_mul_crt_poly_assign — glwe/dcrt.rs:178-255; DcrtGlev::mul_crt_poly_to — glev/dcrt.rs:45-110 */
int pfhe_extprod32_add_dcrt_glev_mul_crt_poly_assign_dev(pfhe_extprod32_plan *plan, uint32_t *acc_dev, size_t len_acc,
                                                         const uint32_t *dcrt_glev_dev, size_t len_glev,
                                                         const uint32_t *crt_poly_dev, size_t len_poly, void *stream);
int pfhe_extprod32_glev_mul_crt_poly_to_dev(pfhe_extprod32_plan *plan, const uint32_t *dcrt_glev_dev, size_t len_glev,
                                            const uint32_t *crt_poly_dev, size_t len_poly, uint32_t *result_dev,
                                            size_t len_result, void *stream);
/* DcrtGlwe::add_dcrt_glev_mul_big_uint_poly_assign — glwe/dcrt.rs:258-338; DcrtGlev::mul_big_uint_poly_to —
 * glev/dcrt.rs:113-175 (the polynomial as big_uint_value_len u32 limbs per coefficient) */
int pfhe_extprod32_add_dcrt_glev_mul_big_uint_poly_assign_dev(pfhe_extprod32_plan *plan, uint32_t *acc_dev, size_t len_acc,
                                                              const uint32_t *dcrt_glev_dev, size_t len_glev,
                                                              const uint32_t *big_uint_poly_dev, size_t len_poly,
                                                              void *stream);
int pfhe_extprod32_glev_mul_big_uint_poly_to_dev(pfhe_extprod32_plan *plan, const uint32_t *dcrt_glev_dev, size_t len_glev,
                                                 const uint32_t *big_uint_poly_dev, size_t len_poly, uint32_t *result_dev,
                                                 size_t len_result, void *stream);

/* The per-element monomial product over U32DcrtTable (as pfhe_dcrt_mul_monomial_each_to_dev, uint32 words). */
int pfhe_dcrt32_mul_monomial_each_to_dev(const pfhe_dcrt32 *table, const uint32_t *a_dev, size_t len,
                                         const uint32_t *exps_dev, size_t polys_per_exp, uint32_t *out_dev, void *stream);
/* The batched blind rotation over the u32 product (as pfhe_blindrot_*, uint32 words; every shape takes the u32 product
 * and one glue launch per step). */
int pfhe_blindrot32_create(const pfhe_dcrt32 *table, const pfhe_rns32 *base, const pfhe_basis32 *basis,
                           size_t glwe_dimension, size_t chunk, pfhe_blindrot32 **out);
void pfhe_blindrot32_destroy(pfhe_blindrot32 *h);
int pfhe_blindrot32_in_use(const pfhe_blindrot32 *h);
size_t pfhe_blindrot32_scratch_bytes(const pfhe_blindrot32 *h);
int pfhe_blindrot32_rotate_dev(pfhe_blindrot32 *h, uint32_t *acc_dev, size_t len_acc, const uint32_t *bsk_dev,
                               size_t len_bsk, const uint32_t *exps_dev, size_t len_exps, void *stream);
int pfhe_blindrot32_rotate(pfhe_blindrot32 *h, uint32_t *acc, size_t len_acc, const uint32_t *bsk, size_t len_bsk,
                           const uint32_t *exps, size_t len_exps);

/* ---- torus FFT (primus_fft) and the TFHE external product (primus_lattice::tfhe) ----
 * FullComplex64FftTable — primus_fft/src/complex64/table.rs:47-130 (the FftTable trait, table.rs): negacyclic transforms of
 * N = 2^log_n torus words.  Fourier values are complex f64 stored as interleaved (re, im) doubles, N per polynomial
 * (fourier_length == poly_length, the reference's full layout); lengths below count complex values.  1 <= log_n <= 14
 * (the N/2-point transform of a polynomial lives in LDS): 0 or more gives PFHE_ERR_UNSUPPORTED, before the device is
 * touched.  u64 names carry no suffix, u32 names end in 32 (TorusFftValue for u64 / u32, primus_fft/src/torus.rs:32-58). */
typedef struct pfhe_fft pfhe_fft;
int pfhe_fft_create(uint32_t log_n, int device, pfhe_fft **out);
void pfhe_fft_destroy(pfhe_fft *fft);
size_t pfhe_fft_poly_length(const pfhe_fft *fft);
size_t pfhe_fft_fourier_length(const pfhe_fft *fft);   /* N, as FullComplex64FftTable */
/* FftTable::forward_torus_slice / inverse_torus_slice over count polynomials (len_input = count*N words -> count*N complex
 * values, and back).  The inverse takes Re of the full inverse, rounds half away from zero and wraps as
 * from_f64_wrapping_rounded (u32: saturate at +-2^63, then mod 2^32; u64: saturate at +-2^127, then exactly mod 2^64) on any
 * spectrum, conjugate-symmetric or not. */
int pfhe_fft_forward_torus_dev(const pfhe_fft *fft, const uint64_t *input_dev, size_t len_input, double *output_dev,
                               size_t len_output, void *stream);
int pfhe_fft_forward_torus32_dev(const pfhe_fft *fft, const uint32_t *input_dev, size_t len_input, double *output_dev,
                                 size_t len_output, void *stream);
int pfhe_fft_inverse_torus_dev(const pfhe_fft *fft, const double *input_dev, size_t len_input, uint64_t *output_dev,
                               size_t len_output, void *stream);
int pfhe_fft_inverse_torus32_dev(const pfhe_fft *fft, const double *input_dev, size_t len_input, uint32_t *output_dev,
                                 size_t len_output, void *stream);
/* host-slice forms of the same four (the trait's own signatures; staged, synchronous) */
int pfhe_fft_forward_torus_slice(const pfhe_fft *fft, const uint64_t *input, size_t len_input, double *output,
                                 size_t len_output);
int pfhe_fft_forward_torus32_slice(const pfhe_fft *fft, const uint32_t *input, size_t len_input, double *output,
                                   size_t len_output);
int pfhe_fft_inverse_torus_slice(const pfhe_fft *fft, const double *input, size_t len_input, uint64_t *output,
                                 size_t len_output);
int pfhe_fft_inverse_torus32_slice(const pfhe_fft *fft, const double *input, size_t len_input, uint32_t *output,
                                   size_t len_output);

/* The plan of the TFHE product: ApproxSignedBasis<T>::new(None, log_basis, Some(decompose_length) or None)
 * (primus_decompose/src/primitive/basis.rs:47-177; decompose_length 0 = the full BITS / log_basis) bundled with
 * TfheFftContext<T> (primus_lattice/src/context/tfhe.rs).  The basis's assert!s (log_basis in 1..BITS-1, decompose_length
 * at most BITS / log_basis) give PFHE_ERR_BAD_ARGUMENT before anything else is looked at; glwe_dimension (k) above 64 gives
 * PFHE_ERR_UNSUPPORTED.  `fft` is borrowed and must outlive the plan.  k = 1 with N <= 2^11 runs one fused launch per
 * chunk and owns no scratch; every other shape owns chunk*(k+1)*(ell+1)*N/2 + (k+1)*ell*(k+1)*N/2 complex values of device
 * scratch (chunk 0 = about 256 MiB).  Everything is allocated here; a call only queues work, so it can be captured into a
 * HIP graph.  One holder at a time (PFHE_ERR_BUSY), successive calls on different streams ordered by the plan, as
 * pfhe_extprod_plan. */
typedef struct pfhe_tfhe_plan pfhe_tfhe_plan;
typedef struct pfhe_tfhe32_plan pfhe_tfhe32_plan;
int pfhe_tfhe_plan_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                          size_t chunk, pfhe_tfhe_plan **out);
void pfhe_tfhe_plan_destroy(pfhe_tfhe_plan *plan);
int pfhe_tfhe_plan_in_use(const pfhe_tfhe_plan *plan);  /* 1 while some thread is inside a call on it */
size_t pfhe_tfhe_plan_scratch_bytes(const pfhe_tfhe_plan *plan);
/* external_product_to — primus_lattice/src/tfhe/external_product.rs:36-93: output = input (x) key for a batch of GLWE
 * ciphertexts (len_input = len_output = batch*(k+1)*N torus words; the same buffer or disjoint) and ONE Fourier GGSW key
 * in the reference's layout, (k+1) rows x ell levels x (k+1) components x N complex values (len_key counts them).  Results
 * are deterministic and do not depend on the batch size or the chunk. */
int pfhe_tfhe_external_product_to_dev(pfhe_tfhe_plan *plan, const uint64_t *input_dev, size_t len_input,
                                      const double *key_dev, size_t len_key, uint64_t *output_dev, size_t len_output,
                                      void *stream);
int pfhe_tfhe_external_product_to(pfhe_tfhe_plan *plan, const uint64_t *input, size_t len_input, const double *key,
                                  size_t len_key, uint64_t *output, size_t len_output);
int pfhe_tfhe32_plan_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                            size_t chunk, pfhe_tfhe32_plan **out);
void pfhe_tfhe32_plan_destroy(pfhe_tfhe32_plan *plan);
int pfhe_tfhe32_plan_in_use(const pfhe_tfhe32_plan *plan);
size_t pfhe_tfhe32_plan_scratch_bytes(const pfhe_tfhe32_plan *plan);
int pfhe_tfhe32_external_product_to_dev(pfhe_tfhe32_plan *plan, const uint32_t *input_dev, size_t len_input,
                                        const double *key_dev, size_t len_key, uint32_t *output_dev, size_t len_output,
                                        void *stream);
int pfhe_tfhe32_external_product_to(pfhe_tfhe32_plan *plan, const uint32_t *input, size_t len_input, const double *key,
                                    size_t len_key, uint32_t *output, size_t len_output);

/* Batched blind rotation over the TFHE product — the CMUX loop of a programmable bootstrap on torus words.  For every step
 * i = 0 .. n_steps-1 in order, and every ciphertext e of the batch:
 *   D     = X^{exps[e*n_steps+i]} * ACC_e - ACC_e    the monic-monomial rotation of CrtGlwe::mul_monic_monomial_assign
 *                                                    (glwe/crt.rs:76-114) on torus words, sub_element_wise_assign
 *                                                    (macros/mod.rs:438), wrapping modulo 2^BITS
 *   E     = external_product_to(D, BSK_i)            tfhe/external_product.rs:36-93, exactly as
 *                                                    pfhe_tfhe*_external_product_to_dev
 *   ACC_e = ACC_e + E                                add_element_wise_assign (macros/mod.rs:410), wrapping
 * acc: batch GLWE ciphertexts ((k+1) x N torus words each), read and written in place; bsk: n_steps Fourier GGSW keys end
 * to end in the reference's layout ((k+1) x ell x (k+1) x N complex values each; len_bsk counts complex values), shared by
 * the batch; exps: batch x n_steps uint32, ciphertext-major.  PFHE_ERR_BAD_LENGTH unless both lengths divide evenly and
 * len_exps == batch * n_steps; n_steps == 0 is a no-op.  Results are deterministic and do not depend on the batch size or
 * the chunk.
 * create takes the arguments of pfhe_tfhe_plan_create and checks them in the same order (the basis's assert!s first, then
 * PFHE_ERR_UNSUPPORTED for k > 64, then the table).  The handle borrows `fft` and owns a product plan; everything is
 * allocated here, a call only queues work on `stream` (no allocation, no host synchronisation), so one whole rotation can
 * be captured into a HIP graph.  One holder at a time (PFHE_ERR_BUSY), successive calls on different streams ordered.
 * k = 1 with N <= 2^11 runs ONE launch per chunk: a workgroup per ciphertext keeps ACC in LDS across all steps and runs
 * the fused product's own arithmetic per step (PFHE_DISABLE_FUSED_TFHE_BLINDROT, read here, selects the other form).
 * Every other shape runs the product's launches plus one glue launch per step and owns three buffers of chunk
 * ciphertexts (chunk 0: the plan's chunk, capped at about 256 MiB of glue buffers). */
typedef struct pfhe_tfhe_blindrot pfhe_tfhe_blindrot;
typedef struct pfhe_tfhe32_blindrot pfhe_tfhe32_blindrot;
int pfhe_tfhe_blindrot_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                              size_t chunk, pfhe_tfhe_blindrot **out);
void pfhe_tfhe_blindrot_destroy(pfhe_tfhe_blindrot *h);
int pfhe_tfhe_blindrot_in_use(const pfhe_tfhe_blindrot *h);  /* 1 while some thread is inside a call on it */
size_t pfhe_tfhe_blindrot_scratch_bytes(const pfhe_tfhe_blindrot *h);
/* Device form: every exponent is taken modulo 2N on the device. */
int pfhe_tfhe_blindrot_rotate_dev(pfhe_tfhe_blindrot *h, uint64_t *acc_dev, size_t len_acc, const double *bsk_dev,
                                  size_t len_bsk, const uint32_t *exps_dev, size_t len_exps, void *stream);
/* Host form: PFHE_ERR_BAD_ARGUMENT for any exponent of 2N or more (the reference's debug_assert!(r < 2N)). */
int pfhe_tfhe_blindrot_rotate(pfhe_tfhe_blindrot *h, uint64_t *acc, size_t len_acc, const double *bsk, size_t len_bsk,
                              const uint32_t *exps, size_t len_exps);
int pfhe_tfhe32_blindrot_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                size_t chunk, pfhe_tfhe32_blindrot **out);
void pfhe_tfhe32_blindrot_destroy(pfhe_tfhe32_blindrot *h);
int pfhe_tfhe32_blindrot_in_use(const pfhe_tfhe32_blindrot *h);
size_t pfhe_tfhe32_blindrot_scratch_bytes(const pfhe_tfhe32_blindrot *h);
int pfhe_tfhe32_blindrot_rotate_dev(pfhe_tfhe32_blindrot *h, uint32_t *acc_dev, size_t len_acc, const double *bsk_dev,
                                    size_t len_bsk, const uint32_t *exps_dev, size_t len_exps, void *stream);
int pfhe_tfhe32_blindrot_rotate(pfhe_tfhe32_blindrot *h, uint32_t *acc, size_t len_acc, const double *bsk, size_t len_bsk,
                                const uint32_t *exps, size_t len_exps);
/* X^{exps[e]} * element e for a batch of elements of `polys_per_exp` torus polynomials each (len = elements *
 * polys_per_exp * N words; exponents taken modulo 2N) — the per-ciphertext X^{-b_e} * TV that starts a bootstrap; the torus
 * counterpart of pfhe_dcrt_mul_monomial_each_to_dev (CrtGlwe::mul_monic_monomial_assign, glwe/crt.rs:76-114).  out_dev must
 * not overlap a_dev. */
int pfhe_tfhe_mul_monomial_each_to_dev(const pfhe_fft *fft, const uint64_t *a_dev, size_t len, const uint32_t *exps_dev,
                                       size_t polys_per_exp, uint64_t *out_dev, void *stream);
int pfhe_tfhe32_mul_monomial_each_to_dev(const pfhe_fft *fft, const uint32_t *a_dev, size_t len, const uint32_t *exps_dev,
                                         size_t polys_per_exp, uint32_t *out_dev, void *stream);

/* Multi-bit blind rotation over the TFHE product — no reference counterpart (the reference has no bootstrap); the LWE mask is
 * consumed g = grouping_factor elements at a time (1 <= g <= 4), so the serial depth and the transform count of a rotation
 * fall by g.  ASSUMES BINARY LWE KEYS.  The key `bsk` is groups x 2^g Fourier GGSW keys end to end, each in the layout
 * pfhe_tfhe*_blindrot_rotate_dev takes; key [t][j] encrypts prod_b (bit b of j ? s_{t*g+b} : 1 - s_{t*g+b}), the indicator
 * that the key bits of group t equal pattern j.  With n_mask = groups*g, for every ciphertext e and every group t in order:
 *   r_j   = (sum over the set bits b of j of (exps[e*n_mask + t*g + b] mod 2N)) mod 2N,   j = 0 .. 2^g-1,  r_0 = 0
 *   K_e,t = sum_j M(r_j) (.) BSK[t][j]      M(r)[k'] = root[(r*(1-2k')) mod 2N], the spectrum of X^r in the table's full
 *                                           layout; root[i] = tw[i] for i < N, -tw[i-N] otherwise (the table's cis(pi i/N))
 *   ACC_e = external_product_to(ACC_e, K_e,t)     the product itself (no "+ ACC"), wrapping modulo 2^BITS
 * The product only sees a key's Hermitian part and M(r) is Hermitian-symmetric, so the arithmetic is DEFINED on
 * half-spectrum slots: Kh[m] = sum_j M(r_j)[2m] * Herm(BSK[t][j])[2m] with Herm as the product forms it, j ascending, the
 * j = 0 term added without a multiplication and every complex multiply-add a fixed sequence of fused multiply-adds; the
 * product's multiply-accumulate, inverse and torus wrap follow as in pfhe_tfhe*_external_product_to_dev.  Every form below
 * gives the same words, and results do not depend on the batch size or the chunk.
 * acc: batch GLWE ciphertexts, read and written in place; exps: batch x n_mask uint32, ciphertext-major.
 * PFHE_ERR_BAD_LENGTH unless len_acc = batch*(k+1)*N, len_bsk = groups*2^g*key_len and len_exps = batch*groups*g;
 * groups == 0 is a no-op.
 * create runs pfhe_tfhe_plan_create's checks first, in its order (the basis's assert!s, PFHE_ERR_UNSUPPORTED for k > 64, the
 * table), then PFHE_ERR_BAD_ARGUMENT for grouping_factor outside 1..4 — all before the device is touched.  The handle
 * borrows `fft`; everything is allocated here, a call only queues work on `stream` (no allocation, no host
 * synchronisation), so one whole rotation can be captured into a HIP graph; a batch larger than the chunk runs chunk by
 * chunk.  One holder at a time (PFHE_ERR_BUSY), successive calls on different streams ordered.
 * k = 1 with N <= 2^11 runs ONE launch per chunk: a workgroup per ciphertext keeps ACC in LDS across all groups and forms
 * K_e,t slot by slot inside the fused product's accumulate code (PFHE_DISABLE_FUSED_TFHE_BLINDROT, read here, selects the
 * other form).  Every other shape runs four launches per group (the Hermitian parts of the group's 2^g keys, the digit
 * transforms of ACC, the multiply-accumulate with K_e,t formed per ciphertext, the inverses back into ACC) over scratch of
 * `chunk` ciphertexts (chunk 0: about 256 MiB) plus the Hermitian parts of 2^g keys. */
typedef struct pfhe_tfhe_mbrot pfhe_tfhe_mbrot;
typedef struct pfhe_tfhe32_mbrot pfhe_tfhe32_mbrot;
int pfhe_tfhe_mbrot_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                           size_t grouping_factor, size_t chunk, pfhe_tfhe_mbrot **out);
void pfhe_tfhe_mbrot_destroy(pfhe_tfhe_mbrot *h);
int pfhe_tfhe_mbrot_in_use(const pfhe_tfhe_mbrot *h);  /* 1 while some thread is inside a call on it */
size_t pfhe_tfhe_mbrot_scratch_bytes(const pfhe_tfhe_mbrot *h);
/* Device form: every exponent is taken modulo 2N on the device. */
int pfhe_tfhe_mbrot_rotate_dev(pfhe_tfhe_mbrot *h, uint64_t *acc_dev, size_t len_acc, const double *bsk_dev, size_t len_bsk,
                               const uint32_t *exps_dev, size_t len_exps, void *stream);
/* Host form: PFHE_ERR_BAD_ARGUMENT for any exponent of 2N or more, as pfhe_tfhe_blindrot_rotate. */
int pfhe_tfhe_mbrot_rotate(pfhe_tfhe_mbrot *h, uint64_t *acc, size_t len_acc, const double *bsk, size_t len_bsk,
                           const uint32_t *exps, size_t len_exps);
int pfhe_tfhe32_mbrot_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                             size_t grouping_factor, size_t chunk, pfhe_tfhe32_mbrot **out);
void pfhe_tfhe32_mbrot_destroy(pfhe_tfhe32_mbrot *h);
int pfhe_tfhe32_mbrot_in_use(const pfhe_tfhe32_mbrot *h);
size_t pfhe_tfhe32_mbrot_scratch_bytes(const pfhe_tfhe32_mbrot *h);
int pfhe_tfhe32_mbrot_rotate_dev(pfhe_tfhe32_mbrot *h, uint32_t *acc_dev, size_t len_acc, const double *bsk_dev, size_t len_bsk,
                                 const uint32_t *exps_dev, size_t len_exps, void *stream);
int pfhe_tfhe32_mbrot_rotate(pfhe_tfhe32_mbrot *h, uint32_t *acc, size_t len_acc, const double *bsk, size_t len_bsk,
                             const uint32_t *exps, size_t len_exps);
/* The combined key of ONE ciphertext and ONE group as a key of its own (keys are f64 for both widths): keys_dev holds the
 * group's 2^g keys (len_keys = 2^g*key_len complex values, key_len = (k+1)*ell*(k+1)*N with ell = decompose_length >= 1),
 * exps_dev its g exponents (taken modulo 2N), out_dev one key in the reference's full layout: out[2m] = Kh[m],
 * out[(1-2m) mod N] = conj(Kh[m]).  The product's Hermitian step returns Kh[m] from that bit for bit, so the rotation above
 * equals, word for word, this call followed by pfhe_tfhe*_external_product_to_dev per ciphertext and group.
 * In this order: PFHE_ERR_BAD_ARGUMENT for a null table, PFHE_ERR_UNSUPPORTED for glwe_dimension > 64,
 * PFHE_ERR_BAD_ARGUMENT for decompose_length outside 1..64 or g outside 1..4, PFHE_ERR_BAD_LENGTH for lengths that do not
 * fit, PFHE_ERR_BAD_ARGUMENT for a null buffer, for keys_dev or out_dev not aligned to 16 bytes (the kernel loads and
 * stores whole complex values) and for an out_dev that overlaps keys_dev. */
int pfhe_tfhe_mb_combine_key_dev(const pfhe_fft *fft, size_t glwe_dimension, size_t decompose_length, size_t grouping_factor,
                                 const double *keys_dev, size_t len_keys, const uint32_t *exps_dev, size_t len_exps,
                                 double *out_dev, size_t len_out, void *stream);

/* ---- the programmable bootstrap around the blind rotation (u64: no suffix, u32: 32) ----
 * An LWE ciphertext is laid out as the reference's Lwe (primus_lattice/src/lwe/single_message.rs:94-125): a[0..dim) then b,
 * dim + 1 torus words, b = <a,s> + e + m; a batch is ciphertext after ciphertext.  The three stateless steps below are exact
 * integer arithmetic modulo 2^BITS; the two without a table take the device first, as pfhe_memset_dev does.
 *
 * Modulus switch.  NO reference counterpart: the reference has no modulus switching, and the rule is this project's own.
 * With shift = BITS - log_n - 1, sw(w) = (((w >> (shift-1)) + 1) >> 1) & (2N-1): round-to-nearest of w * 2N / 2^BITS, ties
 * up, without overflow; 1 <= log_n <= 14 (PFHE_ERR_BAD_ARGUMENT otherwise).  For every ciphertext e of the batch
 * (len_lwe = batch*(n+1), n = lwe_dimension): exps[e*n + i] = sw(a_{e,i}) — ciphertext-major, what
 * pfhe_tfhe*_blindrot_rotate_dev takes (len_exps = batch*n) — and neg_b[e] = (2N - sw(b_e)) & (2N-1) (len_neg_b = batch). */
int pfhe_tfhe_modswitch_dev(int device, const uint64_t *lwe_dev, size_t len_lwe, size_t lwe_dimension, uint32_t log_n,
                            uint32_t *exps_dev, size_t len_exps, uint32_t *neg_b_dev, size_t len_neg_b, void *stream);
int pfhe_tfhe32_modswitch_dev(int device, const uint32_t *lwe_dev, size_t len_lwe, size_t lwe_dimension, uint32_t log_n,
                              uint32_t *exps_dev, size_t len_exps, uint32_t *neg_b_dev, size_t len_neg_b, void *stream);
/* The strided modulus switch, what a many-LUT rotation takes.  NO reference counterpart.  With
 * v = log_stride, 0 <= v <= log_n:  sw_v(w) = ((((w >> (BITS - log_n - 2 + v)) + 1) >> 1) << v) & (2N-1), i.e. w * 2N / 2^v /
 * 2^BITS rounded to nearest, ties up, times 2^v: every value is a multiple of 2^v, and a word that rounds up to 2N wraps to
 * 0.  exps[e*n + i] = sw_v(a_{e,i}), neg_b[e] = (2N - sw_v(b_e)) & (2N-1); lengths as pfhe_tfhe*_modswitch_dev, whose words
 * sw_0 gives one for one.  Refusals in that call's order, PFHE_ERR_BAD_ARGUMENT for log_stride > log_n right behind log_n's:
 * log_n, log_stride, lwe_dimension, PFHE_ERR_BAD_LENGTH for the lengths, (the empty batch is a no-op,) null pointers, the
 * device. */
int pfhe_tfhe_modswitch_stride_dev(int device, const uint64_t *lwe_dev, size_t len_lwe, size_t lwe_dimension, uint32_t log_n,
                                   uint32_t log_stride, uint32_t *exps_dev, size_t len_exps, uint32_t *neg_b_dev,
                                   size_t len_neg_b, void *stream);
int pfhe_tfhe32_modswitch_stride_dev(int device, const uint32_t *lwe_dev, size_t len_lwe, size_t lwe_dimension, uint32_t log_n,
                                     uint32_t log_stride, uint32_t *exps_dev, size_t len_exps, uint32_t *neg_b_dev,
                                     size_t len_neg_b, void *stream);
/* Sample extraction — Rlwe::extract_lwe_with_index (primus_lattice/src/rlwe/coeff.rs:194-227; index 0: extract_lwe,
 * :264-288) applied to each of the k mask polynomials of a GLWE ciphertext (A_0..A_{k-1}, B): for index h < N the output LWE
 * has dimension k*N, out[j*N + i] = A_j[h - i] for i <= h and -A_j[N + h - i] for i > h (wrapping), out[k*N] = B[h]; its key
 * is the GLWE key polynomials end to end.  len_glwe = batch*(k+1)*N, len_lwe = batch*(k*N+1); 1 <= k <= 64 and index < N
 * (PFHE_ERR_BAD_ARGUMENT otherwise); the output must not overlap the input.  extract_first_few_lwe / MultiMsgLwe:
 * pfhe_tfhe*_sample_extract_first_few and pfhe_tfhe*_multimsg_extract below. */
int pfhe_tfhe_sample_extract_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *glwe_dev, size_t len_glwe,
                                 size_t index, uint64_t *lwe_dev, size_t len_lwe, void *stream);
int pfhe_tfhe_sample_extract(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *glwe, size_t len_glwe, size_t index,
                             uint64_t *lwe, size_t len_lwe);
int pfhe_tfhe32_sample_extract_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *glwe_dev, size_t len_glwe,
                                   size_t index, uint32_t *lwe_dev, size_t len_lwe, void *stream);
int pfhe_tfhe32_sample_extract(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *glwe, size_t len_glwe, size_t index,
                               uint32_t *lwe, size_t len_lwe);
/* LWE key switch — no single reference function; built from reference pieces: a sequence of Lwe::add_mul_scalar_assign
 * (lwe/single_message.rs:262-268) under wrapping arithmetic, with the signed digits of ApproxSignedBasis::init_carry_slice
 * and decompose_iter on the power-of-two modulus (primus_decompose/src/primitive/basis.rs:391-406, primitive/common.rs:226-259;
 * the digit rule of the TFHE product).  With ell = decompose_length (0 = the full BITS / log_basis) the key is
 * in_dimension x ell x (out_dimension+1) words: row (i, j) is an LWE ciphertext of s_i * 2^(drop_bits + j*log_basis) under the
 * output key, levels least significant first.  For every ciphertext e and column c
 *   out[e][c] = [c == out_dimension] * b_e - sum_{i < in_dimension} sum_{j < ell} d_{e,i,j} * ksk[(i*ell + j)*(out_dimension+1) + c]
 * modulo 2^BITS, d_{e,i,.} the digits of a_{e,i}.  ApproxSignedBasis::new's assert!s give PFHE_ERR_BAD_ARGUMENT first, as in
 * pfhe_tfhe_plan_create; then the dimensions (at least 1); then PFHE_ERR_BAD_LENGTH unless len_in = batch*(in_dimension+1),
 * len_ksk = in_dimension*ell*(out_dimension+1) and len_out = batch*(out_dimension+1).  The output must not overlap an input; it
 * may be uninitialised, and a call is repeatable (no atomics). */
int pfhe_tfhe_keyswitch_dev(int device, const uint64_t *lwe_in_dev, size_t len_in, size_t in_dimension, const uint64_t *ksk_dev,
                            size_t len_ksk, size_t out_dimension, uint32_t log_basis, size_t decompose_length,
                            uint64_t *lwe_out_dev, size_t len_out, void *stream);
int pfhe_tfhe_keyswitch(int device, const uint64_t *lwe_in, size_t len_in, size_t in_dimension, const uint64_t *ksk,
                        size_t len_ksk, size_t out_dimension, uint32_t log_basis, size_t decompose_length, uint64_t *lwe_out,
                        size_t len_out);
int pfhe_tfhe32_keyswitch_dev(int device, const uint32_t *lwe_in_dev, size_t len_in, size_t in_dimension,
                              const uint32_t *ksk_dev, size_t len_ksk, size_t out_dimension, uint32_t log_basis,
                              size_t decompose_length, uint32_t *lwe_out_dev, size_t len_out, void *stream);
int pfhe_tfhe32_keyswitch(int device, const uint32_t *lwe_in, size_t len_in, size_t in_dimension, const uint32_t *ksk,
                          size_t len_ksk, size_t out_dimension, uint32_t log_basis, size_t decompose_length, uint32_t *lwe_out,
                          size_t len_out);
/* The bootstrap handle — no reference counterpart as a whole (the reference has no bootstrap); its stages are the calls
 * above around pfhe_tfhe*_blindrot_rotate_dev.  Per chunk of ciphertexts: modulus switch; ACC_e = X^{neg_b[e]} * TV written
 * straight into the handle's accumulator (the rotation of pfhe_tfhe*_mul_monomial_each_to_dev, the test vector read in
 * place); the blind rotation with n_steps = lwe_dimension on the switched exponents; sample extraction at index 0; and, when
 * with_keyswitch is non-zero, the key switch from k*N to lwe_dimension.  With the phase b - <a,s> and BSK_i encrypting s_i the
 * accumulator ends as X^{-phase~} * TV, whose coefficient 0 is TV[phase~] for phase~ < N and -TV[phase~ - N] otherwise.
 *   lwe_in  batch*(n+1) words, n = lwe_dimension;  bsk  n Fourier GGSW keys as pfhe_tfhe*_blindrot_rotate_dev takes them;
 *   tv      a GLWE ciphertext of (k+1)*N words shared by the batch (a trivially encrypted LUT is (0,...,0,tv)), or
 *           batch*(k+1)*N words, one per ciphertext;
 *   ksk     k*N x ks_ell x (n+1) words as pfhe_tfhe*_keyswitch_dev takes them; null with len_ksk 0 without a key switch;
 *   lwe_out batch*(n+1) words, or batch*(k*N+1) without a key switch; it must not overlap an input.
 * create runs the blind rotation's create first and returns its statuses in its order (pfhe_tfhe_blindrot_create), then its
 * own: PFHE_ERR_BAD_ARGUMENT for glwe_dimension 0, lwe_dimension 0 and the key-switch basis's assert!s.  The handle borrows
 * `fft`, owns a blind-rotation handle and, for `chunk` ciphertexts, the accumulator, the exponents, neg_b and (with a key
 * switch) the extracted ciphertexts — everything is allocated here.  chunk 0 is the rotation's default, capped at about
 * 256 MiB of accumulator.  A call only queues work on `stream` (no allocation, no host synchronisation), so one whole
 * bootstrap can be captured into a HIP graph; a batch larger than the chunk runs chunk by chunk, all stages of a chunk
 * first.  One holder at a time (PFHE_ERR_BUSY); PFHE_ERR_BAD_LENGTH for any length that does not fit the others. */
typedef struct pfhe_tfhe_bootstrap_handle pfhe_tfhe_bootstrap_handle;
typedef struct pfhe_tfhe32_bootstrap_handle pfhe_tfhe32_bootstrap_handle;
int pfhe_tfhe_bootstrap_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                               size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length, int with_keyswitch,
                               size_t chunk, pfhe_tfhe_bootstrap_handle **out);
/* The same handle over the multi-bit rotation (pfhe_tfhe_mbrot_*): bsk is then the multi-bit key of
 * (lwe_dimension / grouping_factor) * 2^grouping_factor keys, and every call below works on the handle as before.  The
 * multi-bit rotation's create runs first (its statuses, in its order); PFHE_ERR_BAD_ARGUMENT in addition when lwe_dimension
 * is no multiple of grouping_factor.  Handles made by pfhe_tfhe*_bootstrap_create are not affected. */
int pfhe_tfhe_bootstrap_create_multibit(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                        size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length,
                                        int with_keyswitch, size_t grouping_factor, size_t chunk,
                                        pfhe_tfhe_bootstrap_handle **out);
/* The many-LUT bootstrap on the same handle: ONE rotation per input evaluates 2^log_luts look-ups.  Per
 * chunk: pfhe_tfhe*_modswitch_stride_dev with v = log_luts; the accumulator init as above; the rotation (the classic one for
 * grouping_factor 0 or 1, the multi-bit one above that, on its key); sample extraction of ACC_e at EVERY index i < 2^v, each
 * what pfhe_tfhe*_sample_extract_dev gives at index i; with a key switch, the key switch of all of them.  lwe_out holds
 * batch*2^v ciphertexts, output (e, i) at index e*2^v + i; every other length is as before, and every call below works on
 * the handle.  The words equal, one for one, that composition of public calls; log_luts 0 gives the words of a handle of
 * the two creates above.  The rotated phase is a multiple of 2^v, so with TV[c] = tv_{c mod 2^v}[c - (c mod 2^v)] output i
 * is the ordinary bootstrap of test vector tv_i at the stride-rounded phase.  create, before the device: the rotation's
 * checks in its order (with a grouping factor above 1 its range and PFHE_ERR_BAD_ARGUMENT when lwe_dimension is no multiple
 * of it, as pfhe_tfhe*_bootstrap_create_multibit), then PFHE_ERR_BAD_ARGUMENT for log_luts > log N; then as the creates above. */
int pfhe_tfhe_bootstrap_create_many_lut(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                        size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length,
                                        int with_keyswitch, size_t grouping_factor /* 0 or 1: classic */, uint32_t log_luts,
                                        size_t chunk, pfhe_tfhe_bootstrap_handle **out);
void pfhe_tfhe_bootstrap_destroy(pfhe_tfhe_bootstrap_handle *h);
int pfhe_tfhe_bootstrap_in_use(const pfhe_tfhe_bootstrap_handle *h);  /* 1 while some thread is inside a call on it */
size_t pfhe_tfhe_bootstrap_scratch_bytes(const pfhe_tfhe_bootstrap_handle *h);  /* the rotation handle's scratch included */
int pfhe_tfhe_bootstrap_dev(pfhe_tfhe_bootstrap_handle *h, const uint64_t *lwe_in_dev, size_t len_in, const double *bsk_dev,
                            size_t len_bsk, const uint64_t *tv_dev, size_t len_tv, const uint64_t *ksk_dev, size_t len_ksk,
                            uint64_t *lwe_out_dev, size_t len_out, void *stream);
int pfhe_tfhe_bootstrap(pfhe_tfhe_bootstrap_handle *h, const uint64_t *lwe_in, size_t len_in, const double *bsk, size_t len_bsk,
                        const uint64_t *tv, size_t len_tv, const uint64_t *ksk, size_t len_ksk, uint64_t *lwe_out,
                        size_t len_out);
int pfhe_tfhe32_bootstrap_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                 size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length, int with_keyswitch,
                                 size_t chunk, pfhe_tfhe32_bootstrap_handle **out);
int pfhe_tfhe32_bootstrap_create_multibit(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,
                                          size_t decompose_length, size_t lwe_dimension, uint32_t ks_log_basis,
                                          size_t ks_decompose_length, int with_keyswitch, size_t grouping_factor, size_t chunk,
                                          pfhe_tfhe32_bootstrap_handle **out);
int pfhe_tfhe32_bootstrap_create_many_lut(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,
                                          size_t decompose_length, size_t lwe_dimension, uint32_t ks_log_basis,
                                          size_t ks_decompose_length, int with_keyswitch, size_t grouping_factor,
                                          uint32_t log_luts, size_t chunk, pfhe_tfhe32_bootstrap_handle **out);
void pfhe_tfhe32_bootstrap_destroy(pfhe_tfhe32_bootstrap_handle *h);
int pfhe_tfhe32_bootstrap_in_use(const pfhe_tfhe32_bootstrap_handle *h);
size_t pfhe_tfhe32_bootstrap_scratch_bytes(const pfhe_tfhe32_bootstrap_handle *h);
int pfhe_tfhe32_bootstrap_dev(pfhe_tfhe32_bootstrap_handle *h, const uint32_t *lwe_in_dev, size_t len_in, const double *bsk_dev,
                              size_t len_bsk, const uint32_t *tv_dev, size_t len_tv, const uint32_t *ksk_dev, size_t len_ksk,
                              uint32_t *lwe_out_dev, size_t len_out, void *stream);
int pfhe_tfhe32_bootstrap(pfhe_tfhe32_bootstrap_handle *h, const uint32_t *lwe_in, size_t len_in, const double *bsk, size_t len_bsk,
                          const uint32_t *tv, size_t len_tv, const uint32_t *ksk, size_t len_ksk, uint32_t *lwe_out,
                          size_t len_out);

/* ---- key generation, encryption and phase for the bootstrap above (u64: no suffix, u32: 32) ----
 * NO RANDOM NUMBER IS DRAWN HERE.  Every call is deterministic integer arithmetic modulo 2^BITS on buffers the caller has
 * filled: mask slots hold the uniform words, body slots hold noise + message (pfhe_rand{,32}_fill_rows_dev, at the end of
 * this file, fills them on the device from a ChaCha20 stream).  Keys are arrays of torus words, any words
 * (0/1 for a binary key, all-ones for -1, anything else).  No atomics; a call only queues work on `stream` (no allocation,
 * no host synchronisation) and can be captured into a HIP graph.  The body calls ACCUMULATE into the body slot: a call is
 * repeatable only in that sense (a second call adds the product a second time; add followed by subtract restores the input).
 * Statuses in the house order: argument checks before the device, PFHE_ERR_BAD_LENGTH for lengths that do not divide, then
 * zero ciphertexts as a no-op, then PFHE_ERR_BAD_ARGUMENT for a null pointer; a key must not overlap what is written.
 *
 * LWE body — Lwe::generate_random_zero_sample (primus_lattice/src/lwe/single_message.rs:94-125) without its sampling: for
 * every ciphertext e of the batch (len_lwe = batch*(dimension+1), len_key = dimension, 1 <= dimension <= 2^31-2),
 * b_e <- b_e + <a_e, key>, or b_e <- b_e - <a_e, key> when `subtract` is non-zero.  Adding turns (uniform mask, noise +
 * message) into an encryption; subtracting writes the phase b - <a,s> into the body slot. */
int pfhe_tfhe_lwe_body_mac_dev(int device, uint64_t *lwe_dev, size_t len_lwe, size_t dimension, const uint64_t *key_dev,
                               size_t len_key, int subtract, void *stream);
int pfhe_tfhe_lwe_body_mac(int device, uint64_t *lwe, size_t len_lwe, size_t dimension, const uint64_t *key, size_t len_key,
                           int subtract);
int pfhe_tfhe32_lwe_body_mac_dev(int device, uint32_t *lwe_dev, size_t len_lwe, size_t dimension, const uint32_t *key_dev,
                                 size_t len_key, int subtract, void *stream);
int pfhe_tfhe32_lwe_body_mac(int device, uint32_t *lwe, size_t len_lwe, size_t dimension, const uint32_t *key, size_t len_key,
                             int subtract);
/* GLWE body — Rlwe::generate_random_zero_sample (primus_lattice/src/rlwe/coeff.rs:92-121) without its sampling, for
 * glwe_dimension k in 1..64 (PFHE_ERR_BAD_ARGUMENT otherwise): for every ciphertext (A_0..A_{k-1}, B) of the batch
 * (len_glwe = batch*(k+1)*N), B <- B + sum_j A_j * z_j modulo X^N + 1, exact, or B <- B - ... with `subtract`; key is the k
 * polynomials z_j end to end (len_key = k*N), the layout whose flattening is the key of pfhe_tfhe*_sample_extract's output. */
int pfhe_tfhe_glwe_body_mac_dev(const pfhe_fft *fft, size_t glwe_dimension, uint64_t *glwe_dev, size_t len_glwe,
                                const uint64_t *key_dev, size_t len_key, int subtract, void *stream);
int pfhe_tfhe_glwe_body_mac(const pfhe_fft *fft, size_t glwe_dimension, uint64_t *glwe, size_t len_glwe, const uint64_t *key,
                            size_t len_key, int subtract);
int pfhe_tfhe32_glwe_body_mac_dev(const pfhe_fft *fft, size_t glwe_dimension, uint32_t *glwe_dev, size_t len_glwe,
                                  const uint32_t *key_dev, size_t len_key, int subtract, void *stream);
int pfhe_tfhe32_glwe_body_mac(const pfhe_fft *fft, size_t glwe_dimension, uint32_t *glwe, size_t len_glwe, const uint32_t *key,
                              size_t len_key, int subtract);
/* The gadget term of a torus-form GGSW — no reference counterpart (the reference's GGSW generation samples inside): for a
 * batch of GGSWs of (k+1) x ell x (k+1) x N words each (rows (r, l), levels least significant first) and one message word per
 * GGSW (len_messages = count), m * 2^(drop_bits + l*log_basis) is added to coefficient 0 of component r of row (r, l).
 * pfhe_tfhe_plan_create's checks run first, in its order (the basis's assert!s, PFHE_ERR_UNSUPPORTED for k > 64, the table),
 * then PFHE_ERR_BAD_ARGUMENT for k = 0. */
int pfhe_tfhe_ggsw_add_gadget_dev(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                  uint64_t *ggsw_dev, size_t len_ggsw, const uint64_t *messages_dev, size_t len_messages,
                                  void *stream);
int pfhe_tfhe32_ggsw_add_gadget_dev(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                    uint32_t *ggsw_dev, size_t len_ggsw, const uint32_t *messages_dev, size_t len_messages,
                                    void *stream);
/* The bootstrapping key — no reference counterpart.  ggsw_torus arrives holding the randomness of `keys` GGSWs (masks uniform,
 * bodies noise; len_ggsw = keys*(k+1)*ell*(k+1)*N words).  The call runs the GLWE body call (add) on all rows under glwe_key
 * (k*N words), adds the gadget term of each key's message and runs pfhe_fft_forward_torus*_dev into bsk_out (len_bsk = len_ggsw
 * complex values): on return ggsw_torus is the torus-form key and bsk_out its write_fourier_form, bit for bit.
 *   grouping_factor 0      the layout pfhe_tfhe*_blindrot_rotate_dev / _bootstrap_dev take: keys = n, message of key i = s_i;
 *   grouping_factor 1..4   the layout pfhe_tfhe*_mbrot_rotate_dev takes: keys = (n/g)*2^g, message of key [t][j] =
 *                          prod_b (bit b of j ? s_{t*g+b} : 1 - s_{t*g+b}) in wrapping words, formed on the device;
 * s = lwe_key (n = lwe_dimension words).  After the gadget call's checks: PFHE_ERR_BAD_ARGUMENT for grouping_factor > 4, for n
 * outside 1..2^31-2 and for n % g != 0; then the lengths; then null pointers, ggsw_torus or bsk_out not aligned to 16 bytes,
 * and outputs that overlap each other or a key. */
int pfhe_tfhe_bsk_generate_dev(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                               size_t grouping_factor, const uint64_t *lwe_key_dev, size_t lwe_dimension,
                               const uint64_t *glwe_key_dev, size_t len_glwe_key, uint64_t *ggsw_torus_dev, size_t len_ggsw,
                               double *bsk_out_dev, size_t len_bsk, void *stream);
int pfhe_tfhe32_bsk_generate_dev(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                 size_t grouping_factor, const uint32_t *lwe_key_dev, size_t lwe_dimension,
                                 const uint32_t *glwe_key_dev, size_t len_glwe_key, uint32_t *ggsw_torus_dev, size_t len_ggsw,
                                 double *bsk_out_dev, size_t len_bsk, void *stream);
/* The key-switch key in the layout pfhe_tfhe*_keyswitch_dev takes — no reference counterpart.  ksk arrives holding the
 * randomness of in_dimension x ell rows of out_dimension + 1 words (masks uniform, bodies noise); row (i, j) becomes
 * b <- b + <a, key_out> + key_in[i] * 2^(drop_bits + j*log_basis).  key_in has in_dimension words, key_out out_dimension.
 * ApproxSignedBasis::new's assert!s first, then the dimensions (1..2^31-2), then len_ksk = in_dimension*ell*(out_dimension+1). */
int pfhe_tfhe_ksk_generate_dev(int device, const uint64_t *key_in_dev, size_t in_dimension, const uint64_t *key_out_dev,
                               size_t out_dimension, uint32_t log_basis, size_t decompose_length, uint64_t *ksk_dev,
                               size_t len_ksk, void *stream);
int pfhe_tfhe32_ksk_generate_dev(int device, const uint32_t *key_in_dev, size_t in_dimension, const uint32_t *key_out_dev,
                                 size_t out_dimension, uint32_t log_basis, size_t decompose_length, uint32_t *ksk_dev,
                                 size_t len_ksk, void *stream);

/* ---- packing: LWE ciphertexts back into a GLWE, and multi-message extraction out of one (u64: no suffix, u32: 32) ----
 * Exact integer arithmetic modulo 2^BITS on caller-filled buffers, as the key-generation calls above; no atomics, a call
 * only queues work on `stream` (no allocation, no host synchronisation, no handle), and the table's device is the device.
 *
 * Packing key switch — no reference counterpart (the reference has none, as it has no bootstrap).  `count` LWE ciphertexts
 * of dimension in_dimension become ONE GLWE ciphertext whose message polynomial holds their messages in coefficients
 * 0 .. count-1 (the other coefficients carry no message).  With ell = decompose_length (0 = the full BITS / log_basis):
 *   lwe_in    batch x count x (in_dimension+1) words: ciphertext i of group e is a then b, as pfhe_tfhe*_keyswitch takes them;
 *   pksk      in_dimension x ell x (k+1) x N words: row (j, l) is one GLWE ciphertext (A_1..A_k, B) of
 *             s_j * 2^(drop_bits + l*log_basis) on coefficient 0 under the output key, levels least significant first;
 *   glwe_out  batch x (k+1) x N words, one GLWE per group; it may be uninitialised and must not overlap an input.
 * Modulo 2^BITS and X^N + 1:
 *   out_e = (0, ..., 0, sum_{i<count} b_{e,i} X^i) - sum_{i<count} X^i * sum_{j<in_dimension} sum_{l<ell} d_l(a_{e,i,j}) * pksk[j][l]
 * with d_l the signed digits of ApproxSignedBasis exactly as pfhe_tfhe*_keyswitch_dev forms them (init_carry, decompose_iter,
 * the carry from bit drop_bits-1, the log_basis 1 mask).  With count = 1, sample extraction at index 0 of the result is
 * pfhe_tfhe*_keyswitch against the key whose rows are the index-0 extractions of the pksk rows, word for word.  A call is
 * repeatable, and its result depends neither on the batch size nor on how the kernel tiles the work.
 * Statuses, all before the device is touched: ApproxSignedBasis::new's assert!s (PFHE_ERR_BAD_ARGUMENT) as in
 * pfhe_tfhe_keyswitch_dev; PFHE_ERR_BAD_ARGUMENT for glwe_dimension 0 or above 64 and in_dimension outside 1..2^31-2, for a
 * null table, and for count outside 1..N; PFHE_ERR_BAD_LENGTH unless len_in = batch*count*(in_dimension+1),
 * len_pksk = in_dimension*ell*(k+1)*N and len_out = batch*(k+1)*N; an empty batch is a no-op; then PFHE_ERR_BAD_ARGUMENT for
 * a null pointer or an output that overlaps an input.  This call is exact and serves every shape; the approximate f64 /
 * FFT route for full packings is pfhe_tfhe*_pack_keyswitch_fft_dev below. */
int pfhe_tfhe_pack_keyswitch_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *lwe_in_dev, size_t len_in,
                                 size_t in_dimension, size_t count, const uint64_t *pksk_dev, size_t len_pksk,
                                 uint32_t log_basis, size_t decompose_length, uint64_t *glwe_out_dev, size_t len_out,
                                 void *stream);
int pfhe_tfhe_pack_keyswitch(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *lwe_in, size_t len_in,
                             size_t in_dimension, size_t count, const uint64_t *pksk, size_t len_pksk, uint32_t log_basis,
                             size_t decompose_length, uint64_t *glwe_out, size_t len_out);
int pfhe_tfhe32_pack_keyswitch_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *lwe_in_dev, size_t len_in,
                                   size_t in_dimension, size_t count, const uint32_t *pksk_dev, size_t len_pksk,
                                   uint32_t log_basis, size_t decompose_length, uint32_t *glwe_out_dev, size_t len_out,
                                   void *stream);
int pfhe_tfhe32_pack_keyswitch(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *lwe_in, size_t len_in,
                               size_t in_dimension, size_t count, const uint32_t *pksk, size_t len_pksk, uint32_t log_basis,
                               size_t decompose_length, uint32_t *glwe_out, size_t len_out);
/* The packing key in the layout pfhe_tfhe*_pack_keyswitch_dev takes — no reference counterpart.  pksk arrives holding the
 * randomness of in_dimension x ell GLWE rows (mask polynomials uniform, body polynomials noise); row (j, l) becomes
 *   B <- B + sum_r A_r * z_r + key_in[j] * 2^(drop_bits + l*log_basis)      (the last term on coefficient 0):
 * the GLWE body call (add) on all rows under glwe_key (k*N words), then the message term.  Deterministic; a second call adds
 * the body a second time.  Statuses as pfhe_tfhe*_ksk_generate_dev: ApproxSignedBasis::new's assert!s, then the dimensions
 * (glwe_dimension in 1..64, in_dimension in 1..2^31-2) and the table, then PFHE_ERR_BAD_LENGTH unless len_glwe_key = k*N and
 * len_pksk = in_dimension*ell*(k+1)*N, then null pointers and a key that overlaps pksk. */
int pfhe_tfhe_pksk_generate_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *key_in_dev, size_t in_dimension,
                                const uint64_t *glwe_key_dev, size_t len_glwe_key, uint32_t log_basis, size_t decompose_length,
                                uint64_t *pksk_dev, size_t len_pksk, void *stream);
int pfhe_tfhe32_pksk_generate_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *key_in_dev, size_t in_dimension,
                                  const uint32_t *glwe_key_dev, size_t len_glwe_key, uint32_t log_basis,
                                  size_t decompose_length, uint32_t *pksk_dev, size_t len_pksk, void *stream);
/* Multi-message extraction — Rlwe::extract_first_few_lwe (primus_lattice/src/rlwe/coeff.rs:231-260) applied to each of the k
 * mask polynomials: a GLWE ciphertext (A_0..A_{k-1}, B) becomes the MultiMsgLwe layout of k*N + count words,
 *   multi[j*N] = A_j[0], multi[j*N + i] = -A_j[N - i] for 0 < i < N (wrapping), multi[k*N + h] = B[h] for h < count:
 * the mask of the LWE ciphertext at index 0 once, and the first `count` bodies.  len_glwe = batch*(k+1)*N,
 * len_multi = batch*(k*N+count).  The table, then 1 <= k <= 64 and 1 <= count <= N (PFHE_ERR_BAD_ARGUMENT), as
 * pfhe_tfhe_sample_extract checks its table, dimension and index; then the lengths, the empty batch as a no-op, null
 * pointers, and (device form) an output that overlaps the input. */
int pfhe_tfhe_sample_extract_first_few_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *glwe_dev, size_t len_glwe,
                                           size_t count, uint64_t *multi_dev, size_t len_multi, void *stream);
int pfhe_tfhe_sample_extract_first_few(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *glwe, size_t len_glwe,
                                       size_t count, uint64_t *multi, size_t len_multi);
int pfhe_tfhe32_sample_extract_first_few_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *glwe_dev,
                                             size_t len_glwe, size_t count, uint32_t *multi_dev, size_t len_multi,
                                             void *stream);
int pfhe_tfhe32_sample_extract_first_few(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *glwe, size_t len_glwe,
                                         size_t count, uint32_t *multi, size_t len_multi);
/* The expansion of that layout into `count` LWE ciphertexts of k*N + 1 words per group: ciphertext h is
 * MultiMsgLwe::extract_rlwe_mode(dimension, h) (lwe/multiple_message.rs:250-263) per mask polynomial — the mask rotated
 * right by h with its first h words negated, and the body b_h:
 *   lwe[h][j*N + i] = -multi[j*N + N - h + i] for i < h, multi[j*N + i - h] otherwise;  lwe[h][k*N] = multi[k*N + h],
 * which is pfhe_tfhe*_sample_extract at index h of the GLWE the layout came from, word for word.  len_multi =
 * batch*(k*N+count), len_lwe = batch*count*(k*N+1); statuses as above.  The reference's extract_all is deliberately NOT
 * mirrored: as written it builds its first ciphertext without a body slot and then indexes one past the end
 * (multiple_message.rs:274-281). */
int pfhe_tfhe_multimsg_extract_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *multi_dev, size_t len_multi,
                                   size_t count, uint64_t *lwe_dev, size_t len_lwe, void *stream);
int pfhe_tfhe_multimsg_extract(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *multi, size_t len_multi, size_t count,
                               uint64_t *lwe, size_t len_lwe);
int pfhe_tfhe32_multimsg_extract_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *multi_dev, size_t len_multi,
                                     size_t count, uint32_t *lwe_dev, size_t len_lwe, void *stream);
int pfhe_tfhe32_multimsg_extract(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *multi, size_t len_multi,
                                 size_t count, uint32_t *lwe, size_t len_lwe);

/* ---- the packing key switch in the Fourier domain (u64: no suffix, u32: 32) — opt-in, no reference counterpart ----
 * The same rule as pfhe_tfhe*_pack_keyswitch_dev, computed as ONE external product of in_dimension*ell rows:
 *   D_{j,l}(X) = sum_{i<count} d_l(a_{e,i,j}) X^i;   ACC_c = sum_j sum_l FFT(D_{j,l}) * Herm(FFT(pksk[j][l][c]));
 *   out_e = (0, ..., 0, sum_i b_{e,i} X^i) - IFFT(ACC_c)   modulo 2^BITS and X^N + 1,
 * with the digits exactly as the exact call forms them and the f64 transforms, rounding and torus wrap of
 * pfhe_tfhe*_external_product_to_dev.  APPROXIMATE as that product is: bit-equal to the exact call while every sum stays
 * below 2^53 (small keys), otherwise within the f64 transform's error, which u64 full-torus keys make visible.  Cheaper
 * than the exact call when count approaches N; the exact call stays the default and serves every other shape.
 * Shapes: 1 <= log N <= 11 and 1 <= glwe_dimension <= 3.
 *
 * The plan owns the partial-sum scratch of `chunk` groups (chunk x ceil(in_dimension/4) x (k+1) x N/2 complex values;
 * chunk 0 = what fits 256 MiB, at most 65535), allocated at creation; a call only queues work on its stream, and a batch
 * above the chunk runs chunk by chunk.  One holder at a time (PFHE_ERR_BUSY for a second thread); successive calls on
 * different streams are ordered by the plan.  The mask words are summed in slices of 4, a constant of the build, and the
 * slices in ascending order: a group's result is bit-identical whatever batch or chunk it sits in, and a call repeatable.
 * plan_create, all before the device is touched: ApproxSignedBasis::new's assert!s (PFHE_ERR_BAD_ARGUMENT) as
 * pfhe_tfhe_plan_create; PFHE_ERR_UNSUPPORTED for glwe_dimension above 3, PFHE_ERR_BAD_ARGUMENT for a null table,
 * PFHE_ERR_UNSUPPORTED for log N above 11; PFHE_ERR_BAD_ARGUMENT for glwe_dimension 0 or in_dimension outside 1..2^31-2. */
typedef struct pfhe_tfhe_packfft_plan pfhe_tfhe_packfft_plan;
typedef struct pfhe_tfhe32_packfft_plan pfhe_tfhe32_packfft_plan;
int pfhe_tfhe_packfft_plan_create(const pfhe_fft *fft, size_t glwe_dimension, size_t in_dimension, uint32_t log_basis,
                                  size_t decompose_length, size_t chunk, pfhe_tfhe_packfft_plan **out);
void pfhe_tfhe_packfft_plan_destroy(pfhe_tfhe_packfft_plan *plan);
int pfhe_tfhe_packfft_plan_in_use(const pfhe_tfhe_packfft_plan *plan);
size_t pfhe_tfhe_packfft_plan_scratch_bytes(const pfhe_tfhe_packfft_plan *plan);
int pfhe_tfhe32_packfft_plan_create(const pfhe_fft *fft, size_t glwe_dimension, size_t in_dimension, uint32_t log_basis,
                                    size_t decompose_length, size_t chunk, pfhe_tfhe32_packfft_plan **out);
void pfhe_tfhe32_packfft_plan_destroy(pfhe_tfhe32_packfft_plan *plan);
int pfhe_tfhe32_packfft_plan_in_use(const pfhe_tfhe32_packfft_plan *plan);
size_t pfhe_tfhe32_packfft_plan_scratch_bytes(const pfhe_tfhe32_packfft_plan *plan);
/* The Fourier packing key: pksk in exactly the layout pfhe_tfhe*_pksk_generate_dev writes (in_dimension x ell x (k+1) x N
 * words) becomes the HALF spectrum of every key polynomial in natural order, in_dimension x ell x (k+1) x N/2 complex values
 * (len_fkey counts complex values): fkey[p][i] = FFT_N(centred(pksk[p]) psi)[2i], which for a real polynomial is its
 * Hermitian part, so no per-call Hermitian pass is needed and the key is half the bytes of the reference's full layout.
 * Deterministic.  A null plan (PFHE_ERR_BAD_ARGUMENT), the two lengths (PFHE_ERR_BAD_LENGTH), null pointers, an output
 * that overlaps the input or is not 16-byte aligned (PFHE_ERR_BAD_ARGUMENT). */
int pfhe_tfhe_packfft_key_dev(pfhe_tfhe_packfft_plan *plan, const uint64_t *pksk_dev, size_t len_pksk, double *fkey_dev,
                              size_t len_fkey, void *stream);
int pfhe_tfhe32_packfft_key_dev(pfhe_tfhe32_packfft_plan *plan, const uint32_t *pksk_dev, size_t len_pksk, double *fkey_dev,
                                size_t len_fkey, void *stream);
/* The packing call.  lwe_in and glwe_out have the lengths and layouts of pfhe_tfhe*_pack_keyswitch_dev; fkey is the key
 * above.  Statuses in the exact call's order, behind a null plan (PFHE_ERR_BAD_ARGUMENT): count outside 1..N
 * (PFHE_ERR_BAD_ARGUMENT); PFHE_ERR_BAD_LENGTH unless len_in = batch*count*(in_dimension+1),
 * len_fkey = in_dimension*ell*(k+1)*N/2 and len_out = batch*(k+1)*N; an empty batch is a no-op; then PFHE_ERR_BAD_ARGUMENT
 * for a null pointer and (device form) an output that overlaps an input.  The host form stages its buffers through the
 * host layer all torus calls share. */
int pfhe_tfhe_pack_keyswitch_fft_dev(pfhe_tfhe_packfft_plan *plan, const uint64_t *lwe_in_dev, size_t len_in, size_t count,
                                     const double *fkey_dev, size_t len_fkey, uint64_t *glwe_out_dev, size_t len_out,
                                     void *stream);
int pfhe_tfhe_pack_keyswitch_fft(pfhe_tfhe_packfft_plan *plan, const uint64_t *lwe_in, size_t len_in, size_t count,
                                 const double *fkey, size_t len_fkey, uint64_t *glwe_out, size_t len_out);
int pfhe_tfhe32_pack_keyswitch_fft_dev(pfhe_tfhe32_packfft_plan *plan, const uint32_t *lwe_in_dev, size_t len_in, size_t count,
                                       const double *fkey_dev, size_t len_fkey, uint32_t *glwe_out_dev, size_t len_out,
                                       void *stream);
int pfhe_tfhe32_pack_keyswitch_fft(pfhe_tfhe32_packfft_plan *plan, const uint32_t *lwe_in, size_t len_in, size_t count,
                                   const double *fkey, size_t len_fkey, uint32_t *glwe_out, size_t len_out);

/* ---- the circuit bootstrap: an LWE ciphertext of a bit becomes a GGSW ciphertext (u64: no suffix, u32: 32) ----
 * No reference counterpart; the rules are this project's own.  Conventions as everywhere on the torus side:
 * the phase is b - <a,s>; ApproxSignedBasis has its levels least significant first, g_l = 2^(drop_bits + l*log_basis); digits
 * are those of pfhe_tfhe*_keyswitch_dev (init_carry, the carry from bit drop_bits-1, the log_basis 1 mask); a torus-form
 * GGSW is [(k+1) rows r][ell levels l][(k+1) components][N] words, as pfhe_tfhe*_ggsw_add_gadget_dev takes it.  Under the
 * phase rule row (r, l) of a GGSW of m is a GLWE ciphertext of f_r(m*g_l), with f_r(x) = -z_r*x for r < k (a polynomial,
 * z_r the r-th key polynomial) and f_k(x) = x on coefficient 0.
 *
 * Private functional key switch — stateless, as pfhe_tfhe*_pack_keyswitch_dev.  With ell = decompose_length (0 = the full
 * BITS / log_basis):
 *   lwe_in  batch x levels x (in_dimension+1) words: ciphertext (e, l) is at index e*levels + l, a then b;
 *   pfksk   (k+1) x (in_dimension+1) x ell GLWE rows of (k+1)*N words: row (u, j, t) encrypts f_u(s'_j * g_t) with
 *           s' = (s_in, -1): the body word is one more mask word whose key is -1 (it is decomposed with the rest, not
 *           added in the clear, because f_u of it is secret for u < k);
 *   out     batch x (k+1) x levels x (k+1)*N words, one GGSW-shaped block per e; it may be uninitialised and must not
 *           overlap an input.
 * Modulo 2^BITS, with c_{e,l} = (a, b) of ciphertext (e, l):
 *   out[e][u][l] = - sum_{j <= in_dimension} sum_{t < ell} d_t(c_{e,l,j}) * pfksk[u][j][t],
 * so that the phase of out[e][u][l] is f_u of the (rounded) phase of ciphertext (e, l).  Exact wrapping integer
 * arithmetic; no atomics, no scratch beyond the kernel's own LDS; a call is repeatable and its result depends neither on
 * the batch size nor on how the kernel tiles the work.  levels = 1 is the plain form: one ciphertext to k+1 GLWE ciphertexts.
 * Statuses, in this order and all before the device is touched: ApproxSignedBasis::new's assert!s (PFHE_ERR_BAD_ARGUMENT);
 * PFHE_ERR_BAD_ARGUMENT for glwe_dimension outside 1..64 or in_dimension outside 1..2^31-2; for a null table; for levels
 * outside 1..64; PFHE_ERR_BAD_LENGTH unless len_in = batch*levels*(in_dimension+1),
 * len_pfksk = (k+1)*(in_dimension+1)*ell*(k+1)*N and len_out = batch*(k+1)*levels*(k+1)*N; an empty batch is a no-op; then
 * PFHE_ERR_BAD_ARGUMENT for a null pointer and, in the device form only, for an output that overlaps an input; only then
 * the device (PFHE_ERR_NO_DEVICE). */
int pfhe_tfhe_private_keyswitch_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *lwe_in_dev, size_t len_in,
                                    size_t in_dimension, size_t levels, const uint64_t *pfksk_dev, size_t len_pfksk,
                                    uint32_t log_basis, size_t decompose_length, uint64_t *out_dev, size_t len_out,
                                    void *stream);
int pfhe_tfhe_private_keyswitch(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *lwe_in, size_t len_in,
                                size_t in_dimension, size_t levels, const uint64_t *pfksk, size_t len_pfksk, uint32_t log_basis,
                                size_t decompose_length, uint64_t *out, size_t len_out);
int pfhe_tfhe32_private_keyswitch_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *lwe_in_dev, size_t len_in,
                                      size_t in_dimension, size_t levels, const uint32_t *pfksk_dev, size_t len_pfksk,
                                      uint32_t log_basis, size_t decompose_length, uint32_t *out_dev, size_t len_out,
                                      void *stream);
int pfhe_tfhe32_private_keyswitch(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *lwe_in, size_t len_in,
                                  size_t in_dimension, size_t levels, const uint32_t *pfksk, size_t len_pfksk,
                                  uint32_t log_basis, size_t decompose_length, uint32_t *out, size_t len_out);
/* The key of that switch, generated as pfhe_tfhe*_pksk_generate_dev generates the packing key: pfksk arrives holding the
 * randomness of (k+1) x (in_dimension+1) x ell GLWE rows (mask polynomials uniform, body polynomials noise).  The GLWE body
 * call (add) runs on all rows under glwe_key (k*N words), then one launch adds the messages, with s'_j = key_in[j] for
 * j < in_dimension and -1 for j = in_dimension:
 *   row (k, j, t):          B[0] <- B[0] + s'_j * g_t;
 *   row (u, j, t), u < k:   B[i] <- B[i] - s'_j * g_t * z_u[i]   for every coefficient i.
 * No random number is drawn; a second call adds body and messages a second time.  Statuses as
 * pfhe_tfhe*_pksk_generate_dev: ApproxSignedBasis::new's assert!s, then the dimensions and the table, then
 * PFHE_ERR_BAD_LENGTH unless len_glwe_key = k*N and len_pfksk = (k+1)*(in_dimension+1)*ell*(k+1)*N, then null pointers and a
 * key that overlaps pfksk. */
int pfhe_tfhe_pfksk_generate_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *key_in_dev, size_t in_dimension,
                                 const uint64_t *glwe_key_dev, size_t len_glwe_key, uint32_t log_basis, size_t decompose_length,
                                 uint64_t *pfksk_dev, size_t len_pfksk, void *stream);
int pfhe_tfhe32_pfksk_generate_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *key_in_dev, size_t in_dimension,
                                   const uint32_t *glwe_key_dev, size_t len_glwe_key, uint32_t log_basis,
                                   size_t decompose_length, uint32_t *pfksk_dev, size_t len_pfksk, void *stream);
/* The circuit bootstrap handle.  An input LWE ciphertext encrypts a bit m as m*2^(BITS-1).  Per chunk of inputs, per input e
 * and level l of the output basis (cbs_log_basis, cbs_decompose_length: ell_cb levels g_l):
 *   1. the modulus switch of pfhe_tfhe*_modswitch_dev on (a, b + 2^(BITS-2)): the switched phase sits a quarter turn from
 *      both sign changes; the exponents of e serve all ell_cb accumulators;
 *   2. ACC_{e,l} = X^{neg_b[e]} * TV_l, TV_l the trivial GLWE whose body has -g_l/2 on every coefficient, written from
 *      constants (no test vector in memory);
 *   3. the blind rotation of pfhe_tfhe*_blindrot_rotate_dev over batch*ell_cb accumulators, through a rotation handle the
 *      circuit bootstrap owns;
 *   4. sample extraction at index 0, and g_l/2 added to the extracted body: the phase is then m*g_l plus noise;
 *   5. the private functional key switch above with levels = ell_cb and in_dimension = k*N into ggsw_out.
 *   lwe_in    batch*(n+1) words, n = lwe_dimension;  bsk  n Fourier GGSW keys as pfhe_tfhe*_blindrot_rotate_dev takes them;
 *   pfksk     (k+1)*(k*N+1)*pfks_ell*(k+1)*N words as pfhe_tfhe*_pfksk_generate_dev writes them for key_in = the k GLWE key
 *             polynomials end to end (the key of an extracted sample);
 *   ggsw_out  batch x (k+1)*ell_cb*(k+1)*N words: a torus-form GGSW of m per input under the GLWE key, in the output basis;
 *             pfhe_fft_forward_torus*_dev of it is what pfhe_tfhe*_external_product_to_dev takes with a plan on that basis.
 *             It must not overlap an input and may be uninitialised.
 * The handle gives, word for word, what the composition of the public calls named above gives.
 * create, everything before the device first: the blind rotation's checks in their order (ApproxSignedBasis::new's assert!s,
 * PFHE_ERR_UNSUPPORTED for glwe_dimension above 64, PFHE_ERR_BAD_ARGUMENT for a null table); then PFHE_ERR_BAD_ARGUMENT for
 * glwe_dimension 0 or lwe_dimension outside 1..2^31-2, for the assert!s of the output basis and of the key switch's basis,
 * and for an output basis with drop_bits 0 (g_l/2 must be a word); then the rotation's create.  The handle borrows `fft`,
 * owns a blind-rotation handle and, for `chunk` inputs (chunk*ell_cb accumulators), the accumulators, the exponents, neg_b
 * and the extracted ciphertexts — everything is allocated here.  chunk 0: the rotation's default, capped at about 256 MiB
 * of accumulators.  A call only queues work on `stream` (no allocation, no host synchronisation), so a whole circuit
 * bootstrap can be captured into a HIP graph; a batch larger than the chunk runs chunk by chunk.  One holder at a time
 * (PFHE_ERR_BUSY).  A call refuses, in this order: a null handle, a second holder, PFHE_ERR_BAD_LENGTH for any length that
 * does not fit the others, (the empty batch is a no-op,) null pointers, a bsk not aligned to 16 bytes, an output that
 * overlaps an input (device form), the device. */
typedef struct pfhe_tfhe_cbs_handle pfhe_tfhe_cbs_handle;
typedef struct pfhe_tfhe32_cbs_handle pfhe_tfhe32_cbs_handle;
int pfhe_tfhe_cbs_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                         size_t lwe_dimension, uint32_t cbs_log_basis, size_t cbs_decompose_length, uint32_t pfks_log_basis,
                         size_t pfks_decompose_length, size_t chunk, pfhe_tfhe_cbs_handle **out);
/* The same handle with options; with both off it is pfhe_tfhe*_cbs_create, word for word, and every call
 * below works on it.
 *   grouping_factor g > 1 (0 or 1: classic): the owned rotation is the multi-bit one and bsk the multi-bit key of
 *     (lwe_dimension / g) * 2^g keys that pfhe_tfhe*_bsk_generate_dev writes; the other stages are unchanged.
 *   shared_rotation non-zero: ONE rotation per input serves all ell_cb levels.  With v = ceil(log2 ell_cb), per chunk:
 *     1. pfhe_tfhe*_modswitch_stride_dev with v on (a, b + 2^(BITS-2)); exponents and neg_b of an input are written once;
 *     2. ACC_e = X^{neg_b[e]} * TV, TV the trivial GLWE whose body coefficient c is -g_{c mod 2^v}/2 when c mod 2^v < ell_cb
 *        and 0 otherwise, written from constants;
 *     3. the rotation over the chunk's accumulators, one per input;
 *     4. sample extraction of ACC_e at index l for every l < ell_cb, with g_l/2 added to the body, into row e*ell_cb + l;
 *     5. the private functional key switch, as before.
 *     The words equal, one for one, that composition of public calls (pfhe_tfhe*_mul_monomial_each_to_dev on TV in memory
 *     for step 2); with ell_cb = 1 they are the existing handle's.  The handle then owns chunk accumulators, chunk*n
 *     exponents and chunk*ell_cb extracted ciphertexts, and the rotation is created for chunk accumulators; chunk 0 is the
 *     rotation's default capped at about 256 MiB of accumulators.  The switch rounds every word to a multiple of 2^v, so
 *     the worst-case margin of the switched phase is 2^(v-1)*(n+1) plus the input's own error, in units of 2^BITS/2N,
 *     against N/2; outside it the output is right only statistically.  Nothing is refused on that account.
 * create, everything before the device first, in the order of pfhe_tfhe*_cbs_create with the options' refusals in their
 * places: the rotation's checks (for g > 1 with PFHE_ERR_BAD_ARGUMENT for g above 4 last), PFHE_ERR_BAD_ARGUMENT when
 * lwe_dimension is no multiple of g, the dimensions, the two other bases, drop_bits of the output basis, and
 * PFHE_ERR_BAD_ARGUMENT for ell_cb > N with a shared rotation; then the rotation's create. */
int pfhe_tfhe_cbs_create_with(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                              size_t lwe_dimension, uint32_t cbs_log_basis, size_t cbs_decompose_length,
                              uint32_t pfks_log_basis, size_t pfks_decompose_length, size_t grouping_factor /* 0 or 1: classic */,
                              int shared_rotation, size_t chunk, pfhe_tfhe_cbs_handle **out);
void pfhe_tfhe_cbs_destroy(pfhe_tfhe_cbs_handle *h);
int pfhe_tfhe_cbs_in_use(const pfhe_tfhe_cbs_handle *h);  /* 1 while some thread is inside a call on it */
size_t pfhe_tfhe_cbs_scratch_bytes(const pfhe_tfhe_cbs_handle *h);  /* the rotation handle's scratch included */
int pfhe_tfhe_cbs_dev(pfhe_tfhe_cbs_handle *h, const uint64_t *lwe_in_dev, size_t len_in, const double *bsk_dev, size_t len_bsk,
                      const uint64_t *pfksk_dev, size_t len_pfksk, uint64_t *ggsw_out_dev, size_t len_out, void *stream);
int pfhe_tfhe_cbs(pfhe_tfhe_cbs_handle *h, const uint64_t *lwe_in, size_t len_in, const double *bsk, size_t len_bsk,
                  const uint64_t *pfksk, size_t len_pfksk, uint64_t *ggsw_out, size_t len_out);
int pfhe_tfhe32_cbs_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                           size_t lwe_dimension, uint32_t cbs_log_basis, size_t cbs_decompose_length, uint32_t pfks_log_basis,
                           size_t pfks_decompose_length, size_t chunk, pfhe_tfhe32_cbs_handle **out);
int pfhe_tfhe32_cbs_create_with(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                size_t lwe_dimension, uint32_t cbs_log_basis, size_t cbs_decompose_length,
                                uint32_t pfks_log_basis, size_t pfks_decompose_length, size_t grouping_factor,
                                int shared_rotation, size_t chunk, pfhe_tfhe32_cbs_handle **out);
void pfhe_tfhe32_cbs_destroy(pfhe_tfhe32_cbs_handle *h);
int pfhe_tfhe32_cbs_in_use(const pfhe_tfhe32_cbs_handle *h);
size_t pfhe_tfhe32_cbs_scratch_bytes(const pfhe_tfhe32_cbs_handle *h);
int pfhe_tfhe32_cbs_dev(pfhe_tfhe32_cbs_handle *h, const uint32_t *lwe_in_dev, size_t len_in, const double *bsk_dev,
                        size_t len_bsk, const uint32_t *pfksk_dev, size_t len_pfksk, uint32_t *ggsw_out_dev, size_t len_out,
                        void *stream);
int pfhe_tfhe32_cbs(pfhe_tfhe32_cbs_handle *h, const uint32_t *lwe_in, size_t len_in, const double *bsk, size_t len_bsk,
                    const uint32_t *pfksk, size_t len_pfksk, uint32_t *ggsw_out, size_t len_out);

/* ---- the batched CMUX with a selector per group, and the CMUX tree (u64: no suffix, u32: 32) ----
 * No reference counterpart; the rules are this project's own, built on the arithmetic of
 * pfhe_tfhe*_external_product_to_dev, which they leave bit for bit what it is.  A selector is a Fourier GGSW key in the
 * layout that call takes: (k+1)*ell*(k+1)*N complex values, e.g. pfhe_fft_forward_torus*_dev of a GGSW that
 * pfhe_tfhe*_cbs_dev wrote, under a handle on that output basis.
 *
 * Rule 1, the CMUX.  d0, d1, out: count GLWE ciphertexts of (k+1)*N words; keys: count / per_key keys end to end;
 * per_key >= 1 and count % per_key == 0.  Modulo 2^BITS:
 *   out[i] = d0[i] + external_product_to(d1[i] - d0[i], keys[i / per_key]),
 * so a key of the bit m selects d_m.  The words equal, one for one, those of a wrapping subtraction,
 * pfhe_tfhe*_external_product_to_dev on each group of per_key differences with the group's key, and a wrapping addition.
 * Nothing is atomic: the words depend neither on the batch, nor on the chunk, nor on how per_key tiles the launches.  out
 * may be exactly d0 or exactly d1; any other overlap of out with an input is refused in the device form.
 *
 * Rule 2, the tree of depth d.  table: 2^d GLWE ciphertexts shared by the batch, or batch*2^d of them, input-major (which
 * one follows from len_table; any other length is refused); selectors: batch x d keys, the key of input e and bit j at
 * index e*d + j (the order in which pfhe_tfhe*_cbs_dev on LWE inputs ordered e*d + j, then the forward transform, gives
 * them); out: batch ciphertexts.  Level j = 0..d-1 halves the nodes, bit 0 the least significant bit of the leaf index:
 *   node_{j+1}[e][i] = node_j[e][2i] + external_product_to(node_j[e][2i+1] - node_j[e][2i], selectors[e*d + j]),
 *   node_0[e] = table (shared or input e's),  out[e] = node_d[e][0],
 * so out[e] is leaf sum_j m_{e,j} 2^j.  The tree equals, word for word, d calls of rule 1 with per_key = 2^(d-1-j) and a key
 * stride of d.
 *
 * create, everything before the device first: the product plan's checks in their order (ApproxSignedBasis::new's assert!s,
 * PFHE_ERR_UNSUPPORTED for glwe_dimension above 64, PFHE_ERR_BAD_ARGUMENT for a null table), then PFHE_ERR_BAD_ARGUMENT for
 * a depth outside 1..16.  The handle borrows `fft` and allocates everything here, for `chunk` inputs: two node buffers of
 * chunk*2^(d-1) and chunk*2^(d-2) ciphertexts (the last level writes into out; depth 1 needs none) and, off the fused shape
 * (k = 1, N <= 2^11), a product plan with its scratch and two buffers of chunk*2^(d-1) ciphertexts.  chunk 0: inputs such
 * that these stay near 256 MiB, at least 1.  A call only queues work on `stream` (no allocation, no host
 * synchronisation), so it can be captured into a HIP graph; a batch larger than the chunk runs chunk by chunk, all levels
 * of a chunk first; rule 1 runs at most chunk*2^(d-1) ciphertexts per launch.  One holder at a time (PFHE_ERR_BUSY).  A
 * call refuses, in the order of pfhe_tfhe*_external_product_to_dev: a null handle, a second holder, PFHE_ERR_BAD_LENGTH
 * for any length that does not fit the others (per_key 0 included), (the empty batch is a no-op,) null pointers, a pointer
 * not aligned to 16 bytes, an overlap (device form), the device. */
typedef struct pfhe_tfhe_cmux_tree_handle pfhe_tfhe_cmux_tree_handle;
typedef struct pfhe_tfhe32_cmux_tree_handle pfhe_tfhe32_cmux_tree_handle;
int pfhe_tfhe_cmux_tree_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                               size_t depth, size_t chunk, pfhe_tfhe_cmux_tree_handle **out);
void pfhe_tfhe_cmux_tree_destroy(pfhe_tfhe_cmux_tree_handle *h);
int pfhe_tfhe_cmux_tree_in_use(const pfhe_tfhe_cmux_tree_handle *h);  /* 1 while some thread is inside a call on it */
size_t pfhe_tfhe_cmux_tree_scratch_bytes(const pfhe_tfhe_cmux_tree_handle *h);  /* the owned plan's scratch included */
int pfhe_tfhe_cmux_dev(pfhe_tfhe_cmux_tree_handle *h, const uint64_t *d0_dev, size_t len_d0, const uint64_t *d1_dev, size_t len_d1,
                       const double *keys_dev, size_t len_keys, size_t per_key, uint64_t *out_dev, size_t len_out, void *stream);
int pfhe_tfhe_cmux(pfhe_tfhe_cmux_tree_handle *h, const uint64_t *d0, size_t len_d0, const uint64_t *d1, size_t len_d1,
                   const double *keys, size_t len_keys, size_t per_key, uint64_t *out, size_t len_out);
int pfhe_tfhe_cmux_tree_dev(pfhe_tfhe_cmux_tree_handle *h, const uint64_t *table_dev, size_t len_table,
                            const double *selectors_dev, size_t len_selectors, uint64_t *out_dev, size_t len_out, void *stream);
int pfhe_tfhe_cmux_tree(pfhe_tfhe_cmux_tree_handle *h, const uint64_t *table, size_t len_table, const double *selectors,
                        size_t len_selectors, uint64_t *out, size_t len_out);
int pfhe_tfhe32_cmux_tree_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                 size_t depth, size_t chunk, pfhe_tfhe32_cmux_tree_handle **out);
void pfhe_tfhe32_cmux_tree_destroy(pfhe_tfhe32_cmux_tree_handle *h);
int pfhe_tfhe32_cmux_tree_in_use(const pfhe_tfhe32_cmux_tree_handle *h);
size_t pfhe_tfhe32_cmux_tree_scratch_bytes(const pfhe_tfhe32_cmux_tree_handle *h);
int pfhe_tfhe32_cmux_dev(pfhe_tfhe32_cmux_tree_handle *h, const uint32_t *d0_dev, size_t len_d0, const uint32_t *d1_dev,
                         size_t len_d1, const double *keys_dev, size_t len_keys, size_t per_key, uint32_t *out_dev,
                         size_t len_out, void *stream);
int pfhe_tfhe32_cmux(pfhe_tfhe32_cmux_tree_handle *h, const uint32_t *d0, size_t len_d0, const uint32_t *d1, size_t len_d1,
                     const double *keys, size_t len_keys, size_t per_key, uint32_t *out, size_t len_out);
int pfhe_tfhe32_cmux_tree_dev(pfhe_tfhe32_cmux_tree_handle *h, const uint32_t *table_dev, size_t len_table,
                              const double *selectors_dev, size_t len_selectors, uint32_t *out_dev, size_t len_out,
                              void *stream);
int pfhe_tfhe32_cmux_tree(pfhe_tfhe32_cmux_tree_handle *h, const uint32_t *table, size_t len_table, const double *selectors,
                          size_t len_selectors, uint32_t *out, size_t len_out);

/* ---- GLWE key switch, Galois automorphism and homomorphic trace; their keys; the LWE embedding ----
 *
 * All 22 entry points below are the project's own rules, DESIGN.md section 21: the reference has no counterpart.  They are
 * stated over the arithmetic of pfhe_tfhe*_external_product_to_dev, which they leave bit for bit what it is.  Phase is
 * B - sum_j A_j z_j; a GLWE ciphertext is A_0..A_{k-1}, B of N words each; levels are least significant first,
 * g_l = 2^(drop_bits + l*log_basis).  For odd t in 1..2N-1, sigma_t is p(X) -> p(X^t) mod X^N + 1, exact on words:
 * sigma_t(p)[i] = p[u] for u < N and -p[u - N] otherwise, u = i * t^-1 mod 2N.
 *
 * Rule 1, the automorphism with its key switch (t = 1: a plain GLWE key switch).  key: one Fourier key of k*ell rows, row
 * (j, l) k+1 polynomials of N complex values in the reference's layout, i.e. the first k*ell rows of what
 * pfhe_tfhe*_external_product_to_dev takes (pfhe_tfhe*_gksk_generate_dev writes such keys).  Modulo 2^BITS:
 *   out[e] = (0, .., 0, sigma_t(B_e)) - to_torus(sum_{j<k} sum_{l<ell} d_l(sigma_t(A_{e,j})) * key[j][l]).
 * The words equal, one for one, the exact permutation sigma_t of every polynomial, pfhe_tfhe*_external_product_to_dev
 * against the key padded with ell all-zero body rows, and the wrapping subtraction of that from (0, .., 0, sigma_t(B)).
 * Nothing is atomic: the words depend neither on the batch nor on the chunk.  out may not overlap in (the operation is a
 * gather; refused in the device form).  t even or outside 1..2N-1: PFHE_ERR_BAD_ARGUMENT.
 *
 * Rule 2, the trace of `steps` = m steps, 1 <= m <= log N (anything else: PFHE_ERR_BAD_ARGUMENT).  keys: m keys of rule 1
 * end to end, key s-1 for t_s = 2^(log N - s + 1) + 1 (t_1 = N + 1):
 *   ACC_0 = in[e],  ACC_s = ACC_{s-1} + automorphism(ACC_{s-1}, keys[s-1], t_s)  (s = 1..m),  out[e] = ACC_m,
 * word for word m calls of rule 1 with a wrapping addition after each.  The phase of out is 2^m times the phase of in at
 * the coefficients that are multiples of 2^m and (up to key-switch noise) 0 at every other one; m = log N leaves N times
 * coefficient 0.  Dividing the message by 2^m beforehand is the caller's business.  out may be exactly in.
 *
 * Rule 3, the keys (device only, queues work only).  exponents: `count` odd values in 1..2N-1, read on the HOST during the
 * call.  gksk_torus: count x k*ell x (k+1)*N words holding the caller's randomness (mask polynomials uniform, body
 * polynomials noise); row (j, l) of key x becomes B += sum_c A_c (*) key_out_c (pfhe_tfhe*_glwe_body_mac_dev) and
 * B += g_l * sigma_{t_x}(key_in_j); gksk_out: as many complex values, the forward transform of the torus form
 * (pfhe_fft_forward_torus*_dev).  exponents {1}: the key of a plain key switch from key_in to key_out; the t_s of rule 2
 * with key_in == key_out: the trace's keys.  Refused in order: the product plan's checks, glwe_dimension 0, a null or bad
 * exponent, the lengths, (nothing to do,) null pointers, alignment, overlap, the device.
 *
 * Rule 4, the embedding of LWE ciphertexts (a[0..kN), b) into GLWE ciphertexts: A_j[0] = a[jN], A_j[N - i] = -a[jN + i]
 * for i >= 1, B = (b, 0, .., 0); exact, stateless, one thread per output word.  pfhe_tfhe*_sample_extract at index 0
 * returns the LWE ciphertext word for word; followed by the full trace it is the LWE-to-GLWE conversion.
 *
 * create, everything before the device first: the product plan's checks in their order (ApproxSignedBasis::new's assert!s,
 * PFHE_ERR_UNSUPPORTED for glwe_dimension above 64, PFHE_ERR_BAD_ARGUMENT for a null table), then PFHE_ERR_BAD_ARGUMENT for
 * glwe_dimension 0.  The handle borrows `fft` and allocates everything here, for `chunk` ciphertexts (0: a default):
 * nothing on the fused shape (k = 1, N <= 2^11: one launch per chunk for all steps), otherwise the product's scratch and
 * three word buffers of k, 1 and k+1 polynomials per ciphertext.  A call only queues work on `stream` (no allocation, no
 * host synchronisation), so it can be captured into a HIP graph; a batch larger than the chunk runs chunk by chunk, all
 * steps of a chunk first.  One holder at a time (PFHE_ERR_BUSY).  A call refuses: a null handle, a second holder, t or
 * steps out of range, then in the order of pfhe_tfhe*_external_product_to_dev: PFHE_ERR_BAD_LENGTH for any length that does
 * not fit the others, (the empty batch is a no-op,) null pointers, a pointer not aligned to 16 bytes, an overlap (device
 * form), the device. */
typedef struct pfhe_tfhe_glwe_trace_handle pfhe_tfhe_glwe_trace_handle;
typedef struct pfhe_tfhe32_glwe_trace_handle pfhe_tfhe32_glwe_trace_handle;
int pfhe_tfhe_glwe_trace_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                size_t chunk, pfhe_tfhe_glwe_trace_handle **out);
void pfhe_tfhe_glwe_trace_destroy(pfhe_tfhe_glwe_trace_handle *h);
int pfhe_tfhe_glwe_trace_in_use(const pfhe_tfhe_glwe_trace_handle *h);  /* 1 while some thread is inside a call on it */
size_t pfhe_tfhe_glwe_trace_scratch_bytes(const pfhe_tfhe_glwe_trace_handle *h);
int pfhe_tfhe_glwe_automorphism_dev(pfhe_tfhe_glwe_trace_handle *h, const uint64_t *in_dev, size_t len_in, const double *key_dev,
                                    size_t len_key, uint32_t t, uint64_t *out_dev, size_t len_out, void *stream);
int pfhe_tfhe_glwe_automorphism(pfhe_tfhe_glwe_trace_handle *h, const uint64_t *in, size_t len_in, const double *key, size_t len_key,
                                uint32_t t, uint64_t *out, size_t len_out);
int pfhe_tfhe_glwe_trace_dev(pfhe_tfhe_glwe_trace_handle *h, const uint64_t *in_dev, size_t len_in, const double *keys_dev,
                             size_t len_keys, size_t steps, uint64_t *out_dev, size_t len_out, void *stream);
int pfhe_tfhe_glwe_trace(pfhe_tfhe_glwe_trace_handle *h, const uint64_t *in, size_t len_in, const double *keys, size_t len_keys,
                         size_t steps, uint64_t *out, size_t len_out);
int pfhe_tfhe_gksk_generate_dev(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                const uint64_t *key_in_dev, size_t len_key_in, const uint64_t *key_out_dev, size_t len_key_out,
                                const uint32_t *exponents, size_t count, uint64_t *gksk_torus_dev, size_t len_gksk,
                                double *gksk_out_dev, size_t len_out, void *stream);
int pfhe_tfhe_lwe_embed_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *lwe_dev, size_t len_lwe,
                            uint64_t *glwe_out_dev, size_t len_out, void *stream);
int pfhe_tfhe_lwe_embed(const pfhe_fft *fft, size_t glwe_dimension, const uint64_t *lwe, size_t len_lwe, uint64_t *glwe_out,
                        size_t len_out);
int pfhe_tfhe32_glwe_trace_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                  size_t chunk, pfhe_tfhe32_glwe_trace_handle **out);
void pfhe_tfhe32_glwe_trace_destroy(pfhe_tfhe32_glwe_trace_handle *h);
int pfhe_tfhe32_glwe_trace_in_use(const pfhe_tfhe32_glwe_trace_handle *h);
size_t pfhe_tfhe32_glwe_trace_scratch_bytes(const pfhe_tfhe32_glwe_trace_handle *h);
int pfhe_tfhe32_glwe_automorphism_dev(pfhe_tfhe32_glwe_trace_handle *h, const uint32_t *in_dev, size_t len_in, const double *key_dev,
                                      size_t len_key, uint32_t t, uint32_t *out_dev, size_t len_out, void *stream);
int pfhe_tfhe32_glwe_automorphism(pfhe_tfhe32_glwe_trace_handle *h, const uint32_t *in, size_t len_in, const double *key,
                                  size_t len_key, uint32_t t, uint32_t *out, size_t len_out);
int pfhe_tfhe32_glwe_trace_dev(pfhe_tfhe32_glwe_trace_handle *h, const uint32_t *in_dev, size_t len_in, const double *keys_dev,
                               size_t len_keys, size_t steps, uint32_t *out_dev, size_t len_out, void *stream);
int pfhe_tfhe32_glwe_trace(pfhe_tfhe32_glwe_trace_handle *h, const uint32_t *in, size_t len_in, const double *keys, size_t len_keys,
                           size_t steps, uint32_t *out, size_t len_out);
int pfhe_tfhe32_gksk_generate_dev(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                  const uint32_t *key_in_dev, size_t len_key_in, const uint32_t *key_out_dev, size_t len_key_out,
                                  const uint32_t *exponents, size_t count, uint32_t *gksk_torus_dev, size_t len_gksk,
                                  double *gksk_out_dev, size_t len_out, void *stream);
int pfhe_tfhe32_lwe_embed_dev(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *lwe_dev, size_t len_lwe,
                              uint32_t *glwe_out_dev, size_t len_out, void *stream);
int pfhe_tfhe32_lwe_embed(const pfhe_fft *fft, size_t glwe_dimension, const uint32_t *lwe, size_t len_lwe, uint32_t *glwe_out,
                          size_t len_out);

/* ---- ring packing of LWE ciphertexts by automorphisms: the merge and the pack (u64: no suffix, u32: 32) ----
 * The reference has neither; the rules are this project's own (Chen, Dai, Kim, Song, "Efficient homomorphic
 * conversion between (ring) LWE ciphertexts", ACNS 2021, Alg. 3-4), built on rule 1, the trace, their keys and the embedding
 * of the section above, which they leave bit for bit what they are.  Conventions are that section's.  `keys` is the FULL
 * trace's key array: log N keys end to end, keys[s-1] the key of t_s = 2^(log N - s + 1) + 1 (pfhe_tfhe*_gksk_generate_dev
 * with key_in == key_out), whatever the count: no new key, no new format.  The family has a prefix of its own,
 * pfhe_ringpack_ / pfhe_ringpack32_ (as pfhe_bitext_ / pfhe_bitext32_), and the handle types are pfhe_ringpack /
 * pfhe_ringpack32; the u32 prototype of each call is the u64 one with uint64_t -> uint32_t and the handle's 32 name.
 *
 * Rule A, the merge at `level` l, 1 <= l <= log N (anything else: PFHE_ERR_BAD_ARGUMENT), with s = N / 2^l, t = 2^l + 1 and
 * key the key of t.  Modulo 2^BITS:
 *   D = even[e] - X^s odd[e],  S = even[e] + X^s odd[e],  out[e] = S + automorphism(D, key, t).
 * The words equal, one for one, pfhe_tfhe*_mul_monomial_each_to_dev, a wrapping subtraction and addition,
 * pfhe_tfhe*_glwe_automorphism_dev and a wrapping addition.  sigma_t fixes X^j for j a multiple of 2s and negates it for j
 * an odd multiple of s, so out = (even + sigma_t(even)) + X^s (odd + sigma_t(odd)): what either child holds at a multiple
 * of 2s is doubled, what it holds at an odd multiple of s cancels.  out may be exactly even (a node reads both children
 * wholly before it writes); any other overlap, and any overlap with odd or key, is refused in the device form.
 *
 * Rule B, the pack of `count` LWE ciphertexts per output, 1 <= count <= max_count (anything else: PFHE_ERR_BAD_ARGUMENT),
 * m = ceil(log2 count).  lwe: batch*count ciphertexts of k*N + 1 words, group e ciphertexts e*count .. e*count + count - 1:
 *   node_0[i] = embedding of lwe[e*count + i] (rule 4 above) for i < count, the all-zero ciphertext for count <= i < 2^m,
 *   node_l[r] = merge(node_{l-1}[r], node_{l-1}[r + 2^(m-l)], keys[log N - l], level l),  l = 1..m, r < 2^(m-l),
 *   glwe_out[e] = trace(node_m[0], keys[0 .. log N - m), steps = log N - m)     (node_m[0] itself when m = log N),
 * word for word that composition of the public calls, for every shape, batch, chunk and count.  The phase of glwe_out[e] is
 * N times the phase of ciphertext i at coefficient i * N / 2^m and (up to key-switch noise) 0 at every other one: the stride
 * is N / 2^m, where pfhe_tfhe*_pack_keyswitch fills coefficients 0..count-1.  The factor N is NOT removed, as the trace's
 * 2^m is not: the message has to sit log N bits lower in the inputs than it is wanted in the output.  That is the price
 * against the packing key switch, whose key is about 50 times larger.  len_keys is log N * k*ell*(k+1)*N for every count
 * (PFHE_ERR_BAD_LENGTH otherwise); glwe_out may overlap neither lwe nor keys.
 *
 * create, everything before the device first: the product plan's checks in their order, PFHE_ERR_BAD_ARGUMENT for
 * glwe_dimension 0, then for max_count 0 or above N.  The handle borrows `fft` and allocates everything here, for `chunk`
 * OUTPUT ciphertexts (0: a default near 256 MiB): the node buffer of chunk * max(1, 2^(M-1)) GLWE ciphertexts,
 * M = ceil(log2 max_count), and off the fused shape (k = 1, N <= 2^11) the general form's buffers for as many.  On the fused
 * shape a pack is one launch per level and chunk (the LWE leaves are read through the embedding's index rule and never
 * stored; the root runs its trailing trace steps in the same launch), otherwise per level a prepare launch and the
 * trace's general step.  A call only queues work on `stream` (no allocation, no host synchronisation), so it can be
 * captured into a HIP graph; a batch larger than the chunk runs chunk by chunk.  One holder at a time (PFHE_ERR_BUSY).  A
 * call refuses: a null handle, a second holder, level or count out of range, then in the order of
 * pfhe_tfhe*_glwe_trace_dev: PFHE_ERR_BAD_LENGTH for any length that does not fit the others, (the empty batch is a
 * no-op,) null pointers, a pointer not aligned to 16 bytes, an overlap (device form), the device. */
typedef struct pfhe_ringpack pfhe_ringpack;
typedef struct pfhe_ringpack32 pfhe_ringpack32;
int pfhe_ringpack_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                         size_t max_count, size_t chunk, pfhe_ringpack **out);
void pfhe_ringpack_destroy(pfhe_ringpack *h);
int pfhe_ringpack_in_use(const pfhe_ringpack *h);
size_t pfhe_ringpack_scratch_bytes(const pfhe_ringpack *h);
/* rule A: out[e] = S + automorphism(D, key, 2^level + 1), D = even[e] - X^s odd[e], S = even[e] + X^s odd[e], s = N / 2^level */
int pfhe_ringpack_merge_dev(pfhe_ringpack *h, const uint64_t *even_dev, size_t len_even, const uint64_t *odd_dev,
                            size_t len_odd, const double *key_dev, size_t len_key, uint32_t level, uint64_t *out_dev, size_t len_out, void *stream);
int pfhe_ringpack_merge(pfhe_ringpack *h, const uint64_t *even, size_t len_even, const uint64_t *odd, size_t len_odd,
                        const double *key, size_t len_key, uint32_t level, uint64_t *out, size_t len_out);
/* rule B: glwe_out[e] = the pack of LWE ciphertexts e*count .. e*count + count - 1: N phi_i at coefficient i N / 2^m */
int pfhe_ringpack_pack_dev(pfhe_ringpack *h, const uint64_t *lwe_dev, size_t len_lwe, const double *keys_dev,
                           size_t len_keys, size_t count, uint64_t *glwe_out_dev, size_t len_out, void *stream);
int pfhe_ringpack_pack(pfhe_ringpack *h, const uint64_t *lwe, size_t len_lwe, const double *keys, size_t len_keys,
                       size_t count, uint64_t *glwe_out, size_t len_out);
int pfhe_ringpack32_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                           size_t max_count, size_t chunk, pfhe_ringpack32 **out);
void pfhe_ringpack32_destroy(pfhe_ringpack32 *h);
int pfhe_ringpack32_in_use(const pfhe_ringpack32 *h);
size_t pfhe_ringpack32_scratch_bytes(const pfhe_ringpack32 *h);
/* rule A: out[e] = S + automorphism(D, key, 2^level + 1), D = even[e] - X^s odd[e], S = even[e] + X^s odd[e], s = N / 2^level */
int pfhe_ringpack32_merge_dev(pfhe_ringpack32 *h, const uint32_t *even_dev, size_t len_even, const uint32_t *odd_dev,
                              size_t len_odd, const double *key_dev, size_t len_key, uint32_t level, uint32_t *out_dev, size_t len_out, void *stream);
int pfhe_ringpack32_merge(pfhe_ringpack32 *h, const uint32_t *even, size_t len_even, const uint32_t *odd, size_t len_odd,
                          const double *key, size_t len_key, uint32_t level, uint32_t *out, size_t len_out);
/* rule B: glwe_out[e] = the pack of LWE ciphertexts e*count .. e*count + count - 1: N phi_i at coefficient i N / 2^m */
int pfhe_ringpack32_pack_dev(pfhe_ringpack32 *h, const uint32_t *lwe_dev, size_t len_lwe, const double *keys_dev,
                             size_t len_keys, size_t count, uint32_t *glwe_out_dev, size_t len_out, void *stream);
int pfhe_ringpack32_pack(pfhe_ringpack32 *h, const uint32_t *lwe, size_t len_lwe, const double *keys, size_t len_keys,
                         size_t count, uint32_t *glwe_out, size_t len_out);

/* ---- a look-up table on encrypted bits: CMUX tree, rotation by encrypted bits, sample extraction (u64: no suffix, u32: 32) ----
 * The reference has neither; the rules are this project's own, built on the arithmetic of
 * pfhe_tfhe*_external_product_to_dev and on the CMUX above, which they leave bit for bit what they are.  A handle has a
 * tree depth t (0..16), r rotation bits (0..log N), a stride 2^s (r + s <= log N) and o >= 1 outputs; p = t + r >= 1 bits
 * per input, bit 0 the least significant.  A selector is a Fourier GGSW key in the layout the product takes,
 * (k+1)*ell*(k+1)*N complex values.  Bits 0..r-1 drive the rotation, bits r..p-1 the tree.
 *
 * Rule 1, the rotation by encrypted bits.  inp, out: count = batch*o GLWE ciphertexts of (k+1)*N words, accumulator a
 * belonging to input a / o; keys: batch*keys_per_input keys end to end, first_key + r <= keys_per_input.  Modulo 2^BITS:
 *   acc_0 = inp[a],
 *   acc_{j+1} = acc_j + external_product_to(X^{2N - 2^(j+s)} acc_j - acc_j, keys[(a / o)*keys_per_input + first_key + j]),
 *   out[a] = acc_r      (= X^{-x 2^s} inp[a] for key bits x = sum_j m_j 2^j).
 * Per step the words equal, one for one, those of pfhe_tfhe*_mul_monomial_each_to_dev with exponent 2N - 2^(j+s) and then
 * pfhe_tfhe*_cmux_dev(d0 = acc, d1 = the rotated one, the step's keys, per_key = o).  out may be exactly inp; any other
 * overlap is refused in the device form.  r = 0 is a copy.
 *
 * Rule 2, the table.  table: o*2^t GLWE ciphertexts shared by the batch, or batch*o*2^t of them (which one follows from
 * len_table); leaf (output u, index i) of an input at u*2^t + i.  selectors: batch x p keys, the key of input e and bit j
 * at e*p + j (the order in which pfhe_tfhe*_cbs_dev, then the forward transform, leaves them).  Stage A (t > 0): the tree
 * of the CMUX section on the nodes (e, u, i) with bit r + j at level j: t calls of its rule 1 with per_key = o*2^(t-1-j) and
 * a key stride of p keys.  Stage B: rule 1 with keys_per_input = p, first_key = 0 on the batch*o results (t = 0: on the
 * table).  Stage C: with extract = 0, out is the batch*o GLWE ciphertexts; with extract = c in 1..N, batch*o*c LWE
 * ciphertexts of k*N + 1 words, row (e*o + u)*c + i what pfhe_tfhe*_sample_extract_dev writes at index i.  So output (e, u)
 * at index 0 is entry x = sum_j m_{e,j} 2^j of table u when that entry sits in leaf x >> r at body coefficient
 * (x mod 2^r)*2^s.
 *
 * create, everything before the device first and in this order: a null out pointer; the product plan's checks in their order
 * (ApproxSignedBasis::new's assert!s, PFHE_ERR_UNSUPPORTED for glwe_dimension above 64, PFHE_ERR_BAD_ARGUMENT for a null
 * table); PFHE_ERR_BAD_ARGUMENT for tree_depth above 16, for rot_bits + log_stride above log N, for tree_depth + rot_bits = 0,
 * for outputs = 0; PFHE_ERR_BAD_LENGTH for a chunk whose widest launch (chunk*o*2^(t-1) nodes) a grid does not hold.  The
 * handle borrows `fft` and allocates everything here, for `chunk` inputs (0: inputs such that the buffers stay near
 * 256 MiB, at least 1).  A call only queues work on `stream` (no allocation, no host synchronisation), so it can be
 * captured into a HIP graph; a batch larger than the chunk runs chunk by chunk, all stages of a chunk first.  One holder at
 * a time (PFHE_ERR_BUSY).  A call refuses, in the CMUX tree's order: a null handle, a second holder, (rule 2: extract above
 * N,) null pointers (host form), PFHE_ERR_BAD_LENGTH for any length that does not fit the others, (the empty batch is a
 * no-op,) null pointers, a pointer not aligned to 16 bytes, an overlap (device form), the device. */
typedef struct pfhe_tfhe_lut_handle pfhe_tfhe_lut_handle;
typedef struct pfhe_tfhe32_lut_handle pfhe_tfhe32_lut_handle;
int pfhe_tfhe_lut_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                         size_t tree_depth, size_t rot_bits, size_t log_stride, size_t outputs, size_t chunk,
                         pfhe_tfhe_lut_handle **out);
void pfhe_tfhe_lut_destroy(pfhe_tfhe_lut_handle *h);
int pfhe_tfhe_lut_in_use(const pfhe_tfhe_lut_handle *h);  /* 1 while some thread is inside a call on it */
size_t pfhe_tfhe_lut_scratch_bytes(const pfhe_tfhe_lut_handle *h);  /* the owned CMUX buffers and plan included */
int pfhe_tfhe_rotate_by_bits_dev(pfhe_tfhe_lut_handle *h, const uint64_t *inp_dev, size_t len_inp, const double *keys_dev,
                                 size_t len_keys, size_t keys_per_input, size_t first_key, uint64_t *out_dev, size_t len_out,
                                 void *stream);
int pfhe_tfhe_rotate_by_bits(pfhe_tfhe_lut_handle *h, const uint64_t *inp, size_t len_inp, const double *keys, size_t len_keys,
                             size_t keys_per_input, size_t first_key, uint64_t *out, size_t len_out);
int pfhe_tfhe_lut_eval_dev(pfhe_tfhe_lut_handle *h, const uint64_t *table_dev, size_t len_table, const double *selectors_dev,
                           size_t len_selectors, size_t extract, uint64_t *out_dev, size_t len_out, void *stream);
int pfhe_tfhe_lut_eval(pfhe_tfhe_lut_handle *h, const uint64_t *table, size_t len_table, const double *selectors,
                       size_t len_selectors, size_t extract, uint64_t *out, size_t len_out);
int pfhe_tfhe32_lut_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                           size_t tree_depth, size_t rot_bits, size_t log_stride, size_t outputs, size_t chunk,
                           pfhe_tfhe32_lut_handle **out);
void pfhe_tfhe32_lut_destroy(pfhe_tfhe32_lut_handle *h);
int pfhe_tfhe32_lut_in_use(const pfhe_tfhe32_lut_handle *h);
size_t pfhe_tfhe32_lut_scratch_bytes(const pfhe_tfhe32_lut_handle *h);
int pfhe_tfhe32_rotate_by_bits_dev(pfhe_tfhe32_lut_handle *h, const uint32_t *inp_dev, size_t len_inp, const double *keys_dev,
                                   size_t len_keys, size_t keys_per_input, size_t first_key, uint32_t *out_dev, size_t len_out,
                                   void *stream);
int pfhe_tfhe32_rotate_by_bits(pfhe_tfhe32_lut_handle *h, const uint32_t *inp, size_t len_inp, const double *keys,
                               size_t len_keys, size_t keys_per_input, size_t first_key, uint32_t *out, size_t len_out);
int pfhe_tfhe32_lut_eval_dev(pfhe_tfhe32_lut_handle *h, const uint32_t *table_dev, size_t len_table, const double *selectors_dev,
                             size_t len_selectors, size_t extract, uint32_t *out_dev, size_t len_out, void *stream);
int pfhe_tfhe32_lut_eval(pfhe_tfhe32_lut_handle *h, const uint32_t *table, size_t len_table, const double *selectors,
                         size_t len_selectors, size_t extract, uint32_t *out, size_t len_out);

/* ---- bit extraction: an LWE ciphertext of a multi-bit message into one LWE ciphertext per bit (u64: no suffix, u32: 32) ----
 * The reference has none; the rule is this project's own, built from the rules of the LWE key switch, the
 * modulus switch, the accumulator of the circuit bootstrap and the classic blind rotation, which it leaves bit for bit what
 * they are.  It closes the loop of the look-up above: its outputs are what pfhe_tfhe*_cbs_dev takes, in the order in which
 * pfhe_tfhe*_lut_eval_dev expects the selectors.  The family has a prefix of its own, pfhe_bitext_ / pfhe_bitext32_ (as
 * pfhe_blindrot_ / pfhe_blindrot32_ on the RNS side), and the handle types are pfhe_bitext / pfhe_bitext32; the u32 prototype
 * of every pair is the u64 one with uint64_t -> uint32_t and the handle type -> its 32 name.
 *
 * lwe_in: batch ciphertexts of k*N + 1 words under the extracted GLWE key (what pfhe_tfhe*_sample_extract_dev and
 * pfhe_tfhe*_lut_eval_dev with extract >= 1 write), phase b - <a,s> = m*2^delta_log + e.  bits_out: batch*bits ciphertexts of
 * n + 1 words under the LWE key, bit i of input e (bit 0 the least significant) at index e*bits + i, phase
 * m_i*2^(BITS-1) plus noise.  bsk: the n Fourier GGSW keys of pfhe_tfhe*_bootstrap_dev; ksk: the k*N*ks_ell*(n+1) words of
 * pfhe_tfhe*_generate_ksk_dev from the extracted key to the LWE key.  1 <= delta_log, 1 <= bits, delta_log + bits <= BITS;
 * message bits at or above delta_log + bits are shifted out.  With c_0 = lwe_in, for i = 0 .. bits-1, modulo 2^BITS:
 *   bits_out[e*bits + i] = keyswitch(c_i << (BITS - 1 - delta_log - i))     every word shifted as a wrapping word, then the
 *                                                                           rule of pfhe_tfhe*_keyswitch_dev word for word;
 *   unless i = bits-1:  (exps, neg_b) = pfhe_tfhe*_modswitch_dev of that output with 2^(BITS-2) added to its body,
 *                       ACC = X^{neg_b} TV_i, TV_i = (0, .., 0, -2^(delta_log+i-1) on every coefficient),
 *                       ACC rotated by pfhe_tfhe*_blind_rotate_dev over the n keys,
 *                       c_{i+1} = c_i - (pfhe_tfhe*_sample_extract_dev of ACC at index 0, 2^(delta_log+i-1) added to its body).
 * The words equal, one for one, those of that composition of public calls.  lwe_in is read only.
 *
 * create, everything before the device first and in this order: a null out pointer; the product plan's checks in their order
 * (ApproxSignedBasis::new's assert!s, PFHE_ERR_UNSUPPORTED for glwe_dimension above 64, PFHE_ERR_BAD_ARGUMENT for a null
 * table); PFHE_ERR_BAD_ARGUMENT for glwe_dimension 0 or lwe_dimension outside 1..2^31-2; the key-switch basis's assert!s;
 * then the classic rotation's create.  The handle borrows `fft` and allocates everything here, for `chunk` inputs (0: the
 * rotation's default, capped at about 256 MiB of accumulators).  A call only queues work on `stream` (no allocation, no
 * host synchronisation), so it can be captured into a HIP graph; a batch larger than the chunk runs chunk by chunk, all
 * bits of a chunk first.  One holder at a time (PFHE_ERR_BUSY).  A call refuses, in this order: a null handle, a second
 * holder, PFHE_ERR_BAD_ARGUMENT for delta_log = 0, bits = 0 or delta_log + bits above BITS, null pointers (host form),
 * PFHE_ERR_BAD_LENGTH for lwe_in no multiple of k*N + 1, bits_out other than batch*bits*(n+1), bsk other than n keys or ksk
 * other than k*N*ks_ell*(n+1) words, (the empty batch is a no-op,) null pointers, a pointer not aligned to 16 bytes, an
 * output that overlaps an input (device form), the device. */
typedef struct pfhe_bitext pfhe_bitext;
typedef struct pfhe_bitext32 pfhe_bitext32;
int pfhe_bitext_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                            size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length, size_t chunk,
                            pfhe_bitext **out);
void pfhe_bitext_destroy(pfhe_bitext *h);
int pfhe_bitext_in_use(const pfhe_bitext *h);  /* 1 while some thread is inside a call on it */
size_t pfhe_bitext_scratch_bytes(const pfhe_bitext *h);  /* the owned rotation's included */
int pfhe_bitext_extract_bits_dev(pfhe_bitext *h, const uint64_t *lwe_in_dev, size_t len_in, const double *bsk_dev,
                               size_t len_bsk, const uint64_t *ksk_dev, size_t len_ksk, uint32_t delta_log, uint32_t bits,
                               uint64_t *bits_out_dev, size_t len_out, void *stream);
int pfhe_bitext_extract_bits(pfhe_bitext *h, const uint64_t *lwe_in, size_t len_in, const double *bsk, size_t len_bsk,
                           const uint64_t *ksk, size_t len_ksk, uint32_t delta_log, uint32_t bits, uint64_t *bits_out,
                           size_t len_out);
int pfhe_bitext32_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                              size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length, size_t chunk,
                              pfhe_bitext32 **out);
void pfhe_bitext32_destroy(pfhe_bitext32 *h);
int pfhe_bitext32_in_use(const pfhe_bitext32 *h);
size_t pfhe_bitext32_scratch_bytes(const pfhe_bitext32 *h);
int pfhe_bitext32_extract_bits_dev(pfhe_bitext32 *h, const uint32_t *lwe_in_dev, size_t len_in, const double *bsk_dev,
                                 size_t len_bsk, const uint32_t *ksk_dev, size_t len_ksk, uint32_t delta_log, uint32_t bits,
                                 uint32_t *bits_out_dev, size_t len_out, void *stream);
int pfhe_bitext32_extract_bits(pfhe_bitext32 *h, const uint32_t *lwe_in, size_t len_in, const double *bsk,
                             size_t len_bsk, const uint32_t *ksk, size_t len_ksk, uint32_t delta_log, uint32_t bits,
                             uint32_t *bits_out, size_t len_out);

/* ---- linear layer: clear integer weights on batches of LWE ciphertexts (u64: no suffix, u32: 32) ----
 * The leveled step between two bootstraps: out_features chains of Lwe::add_mul_scalar_assign
 * (primus_lattice/src/lwe/single_message.rs:262-268) per input vector, one chain per output, summed over the inputs of a
 * neuron.  The family has a prefix of its own, pfhe_lwe_ / pfhe_lwe32_; the u32 prototype of every pair is
 * the u64 one with uint64_t -> uint32_t.
 *
 * With row = dimension + 1 words per ciphertext (a then b): lwe_in is batch*in_features*row words, vector e, ciphertext i;
 * weights is out_features*in_features scalars, row-major, shared by the batch; bias is out_features words, already encoded
 * as torus words and added to the body, or null with len_bias 0; lwe_out is batch*out_features*row words, may be
 * uninitialised and must not overlap an input.  Modulo 2^BITS:
 *   out[e][o][c] = sum_{i < in_features} W[o][i] * in[e][i][c]  +  [c = dimension] * bias[o]
 * A sum modulo 2^BITS does not depend on its order, so the words depend on no tiling, batch size or path.  The rule is
 * word-wise: a GLWE row of (k+1)*N words passed as dimension = (k+1)*N - 1 with a null bias is served as well.
 *   linear      W[o][i] is a word of the ciphertext's width, the reference's `scalar: T`, a negative weight in two's complement;
 *   linear_i8   W[o][i] is an int8_t; the result is, by definition, linear's on the sign-extended weights (computed on the
 *               matrix cores, byte plane by byte plane; no cap on in_features).
 * Statuses, in this order and all before the device is touched: PFHE_ERR_BAD_ARGUMENT for dimension, in_features or
 * out_features outside 1..2^31-2; PFHE_ERR_BAD_LENGTH unless len_in is a multiple of in_features*row, len_weights =
 * out_features*in_features, len_bias is 0 or out_features and len_out = batch*out_features*row; (an empty batch is a no-op;)
 * PFHE_ERR_BAD_ARGUMENT for a null pointer (a bias of len_bias words included), for a bias pointer with len_bias 0 and for
 * an output that overlaps an input (device form); PFHE_ERR_BAD_LENGTH for more than 2^31-1 workgroups in a row, the batch
 * being folded into one grid dimension with the column tiles: batch*ceil(row/128) for linear, batch*ceil(row/64) for
 * linear_i8 (a status of this implementation, beyond the reference's rule); the device.
 * A call only queues work on `stream`: no allocation, no atomics, no scratch, repeatable, and it can be captured into a
 * HIP graph. */
int pfhe_lwe_linear_dev(int device, const uint64_t *lwe_in_dev, size_t len_in, size_t dimension, const uint64_t *weights_dev,
                        size_t len_weights, size_t in_features, size_t out_features, const uint64_t *bias_dev, size_t len_bias,
                        uint64_t *lwe_out_dev, size_t len_out, void *stream);
int pfhe_lwe_linear(int device, const uint64_t *lwe_in, size_t len_in, size_t dimension, const uint64_t *weights,
                    size_t len_weights, size_t in_features, size_t out_features, const uint64_t *bias, size_t len_bias,
                    uint64_t *lwe_out, size_t len_out);
int pfhe_lwe_linear_i8_dev(int device, const uint64_t *lwe_in_dev, size_t len_in, size_t dimension, const int8_t *weights_dev,
                           size_t len_weights, size_t in_features, size_t out_features, const uint64_t *bias_dev,
                           size_t len_bias, uint64_t *lwe_out_dev, size_t len_out, void *stream);
int pfhe_lwe_linear_i8(int device, const uint64_t *lwe_in, size_t len_in, size_t dimension, const int8_t *weights,
                       size_t len_weights, size_t in_features, size_t out_features, const uint64_t *bias, size_t len_bias,
                       uint64_t *lwe_out, size_t len_out);
int pfhe_lwe32_linear_dev(int device, const uint32_t *lwe_in_dev, size_t len_in, size_t dimension, const uint32_t *weights_dev,
                          size_t len_weights, size_t in_features, size_t out_features, const uint32_t *bias_dev, size_t len_bias,
                          uint32_t *lwe_out_dev, size_t len_out, void *stream);
int pfhe_lwe32_linear(int device, const uint32_t *lwe_in, size_t len_in, size_t dimension, const uint32_t *weights,
                      size_t len_weights, size_t in_features, size_t out_features, const uint32_t *bias, size_t len_bias,
                      uint32_t *lwe_out, size_t len_out);
int pfhe_lwe32_linear_i8_dev(int device, const uint32_t *lwe_in_dev, size_t len_in, size_t dimension, const int8_t *weights_dev,
                             size_t len_weights, size_t in_features, size_t out_features, const uint32_t *bias_dev,
                             size_t len_bias, uint32_t *lwe_out_dev, size_t len_out, void *stream);
int pfhe_lwe32_linear_i8(int device, const uint32_t *lwe_in, size_t len_in, size_t dimension, const int8_t *weights,
                         size_t len_weights, size_t in_features, size_t out_features, const uint32_t *bias, size_t len_bias,
                         uint32_t *lwe_out, size_t len_out);

/* ---- random layer: a device ChaCha20 stream, exact samplers, seeded LWE ciphertexts (u64: no suffix, u32: 32) ----
 * The randomness every encryption call and key generator above takes as a caller-filled buffer (masks uniform, bodies
 * noise), drawn on the device from a position-addressed stream.  The reference's layer is primus_distr,
 * which samples from a stateful `rand::Rng + CryptoRng`; a call here has NO state: output i of a sampler is a closed form
 * of (key, nonce, i), so any call can produce any sub-range and a mask can be re-made from its seed instead of being stored.
 * The families have prefixes of their own, pfhe_csprng_ and pfhe_rand_ / pfhe_rand32_; the u32 prototype of every pair is
 * the u64 one with uint64_t -> uint32_t (keys and nonces are uint32_t words at both widths, indices size_t).
 *
 * The stream: ChaCha20, the 20-round block function of RFC 8439, with a 64-bit block counter in state words 12 (low) and
 * 13 (high) and a 64-bit nonce in words 14 (low) and 15 (high).  `key` points at eight uint32_t words (state words 4..11)
 * and `nonce` at two (words 14, 15), both in HOST memory: a key travels to the kernels as a kernel argument and is never
 * written to device global memory, printed or put into an error message.  u32 stream word j is little-endian word j mod 16
 * of block j div 16; u64 stream word j is u32 words 2j (low half) and 2j+1 (high half).  The layout is RFC 8439 §2.3.2's
 * and `openssl enc -chacha20`'s (whose 16-byte IV is state words 12..15), both tested; it should also be
 * rand_chacha::ChaCha20Rng's (set_stream = the nonce, set_word_pos = the u32 word index, next_u64 low word first), which is
 * UNVERIFIED: no Rust toolchain was at hand.  The library gathers no entropy: the caller supplies every key.
 *
 * Samplers, exact integer rules on u32 / u64 torus words; `offset` is the absolute index of the first output:
 *   keystream  u32 stream words [word_offset, word_offset + n_words) (no primus_distr counterpart: RngCore::next_u32)
 *   uniform    output i = stream word i of the output's width (primus_distr has no power-of-two case: its uniform is
 *              rand's Uniform<T> modulo q, which rejects; sample_uniform_values_to, primus_distr/src/common.rs:87-96)
 *   binary     output i = bit i mod 32 of u32 stream word i div 32: sample_binary_values_to
 *              (primus_distr/src/common.rs:22-42) on the same word stream
 *   ternary    output i = [0, 0, 1, -1][(w >> 2 (i mod 16)) & 3], w = u32 stream word i div 16, -1 the all-ones word:
 *              sample_ternary_values_to (common.rs:56-76)
 *   tuniform   output i takes u64 stream word i at BOTH widths; r = its low bound_log2 + 2 bits; the value is
 *              (r >> 1) + (r & 1) - 2^bound_log2 modulo 2^BITS: support [-2^b, 2^b], the two ends with probability
 *              2^-(b+2), every other value 2^-(b+1), variance (2^(2b+1) + 1) / 6; 0 <= bound_log2 <= BITS - 2 (no
 *              primus_distr counterpart: its noise is the discrete Gaussian, which is out of scope here)
 * Rows: fill_rows writes rows of mask_len + body_len words; for absolute row R = first_row + r (rows = len_out /
 * (mask_len + body_len)) mask word j is uniform output R*mask_len + j of the mask stream, and body word j gets tuniform
 * output R*body_len + j of the noise stream, stored when add = 0 and added otherwise (so messages can be placed first).
 * One launch.  LWE rows are (n, 1), GLWE rows (k*N, N), and the `rand` argument of pfhe_tfhe*_bsk_generate_dev,
 * _ksk_generate_dev, _pksk_generate_dev, _pfksk_generate_dev and _gksk_generate_dev is rows of one of the two (no
 * primus_distr counterpart: the reference draws inside generate_random_zero_sample).
 * Seeded ciphertexts: lwe_encrypt_seeded computes bodies[r] += <mask(R), lwe_key> + noise(R) with mask(R) the row's mask
 * above at mask_len = dimension and noise(R) tuniform output R: the body slot of fill_rows(add) followed by
 * pfhe_tfhe*_lwe_body_mac, word for word, while the mask stays in registers; the key is any words.  seeded_expand writes the
 * full rows, masks from the stream and bodies copied; it takes no noise seed: it is what the receiving side runs (neither
 * has a primus_distr or primus_lattice counterpart).
 * Statuses, in this order and all before the device is touched: PFHE_ERR_BAD_ARGUMENT for a null key or nonce, for
 * (mask_key, mask_nonce) equal to (noise_key, noise_nonce) in the calls that take both (a seeded ciphertext publishes its
 * mask seed, which must never give the noise), for bound_log2 > BITS - 2 and for mask_len, body_len or dimension outside
 * 1..2^31-2; PFHE_ERR_BAD_LENGTH for a length that is not a whole number of rows (len_out, len_bodies; both must give the
 * same rows) and for a last output index above 2^64 - 2^20; (no outputs: a no-op;) PFHE_ERR_BAD_ARGUMENT for a null buffer and, in
 * the device forms, for an output that overlaps an input; PFHE_ERR_BAD_LENGTH for more than 2^31-1 workgroups; the device.
 * A call only queues work on `stream`: no allocation, no atomics, no scratch, repeatable, capturable into a HIP graph. */
int pfhe_csprng_keystream_dev(int device, const uint32_t *key, const uint32_t *nonce, size_t word_offset, uint32_t *out_dev,
                              size_t n_words, void *stream);
int pfhe_rand_uniform_dev(int device, const uint32_t *key, const uint32_t *nonce, size_t offset, uint64_t *out_dev, size_t n,
                          void *stream);
int pfhe_rand_binary_dev(int device, const uint32_t *key, const uint32_t *nonce, size_t offset, uint64_t *out_dev, size_t n,
                         void *stream);
int pfhe_rand_ternary_dev(int device, const uint32_t *key, const uint32_t *nonce, size_t offset, uint64_t *out_dev, size_t n,
                          void *stream);
int pfhe_rand_tuniform_dev(int device, const uint32_t *key, const uint32_t *nonce, size_t offset, uint32_t bound_log2,
                           uint64_t *out_dev, size_t n, void *stream);
int pfhe_rand_fill_rows_dev(int device, const uint32_t *mask_key, const uint32_t *mask_nonce, const uint32_t *noise_key,
                            const uint32_t *noise_nonce, size_t first_row, size_t mask_len, size_t body_len,
                            uint32_t bound_log2, int add, uint64_t *out_dev, size_t len_out, void *stream);
int pfhe_rand_lwe_encrypt_seeded_dev(int device, const uint32_t *mask_key, const uint32_t *mask_nonce,
                                     const uint32_t *noise_key, const uint32_t *noise_nonce, size_t first_row,
                                     const uint64_t *lwe_key_dev, size_t dimension, uint32_t bound_log2, uint64_t *bodies_dev,
                                     size_t rows, void *stream);
int pfhe_rand_lwe_encrypt_seeded(int device, const uint32_t *mask_key, const uint32_t *mask_nonce, const uint32_t *noise_key,
                                 const uint32_t *noise_nonce, size_t first_row, const uint64_t *lwe_key, size_t dimension,
                                 uint32_t bound_log2, uint64_t *bodies, size_t rows);
int pfhe_rand_seeded_expand_dev(int device, const uint32_t *mask_key, const uint32_t *mask_nonce, size_t first_row,
                                size_t mask_len, size_t body_len, const uint64_t *bodies_dev, size_t len_bodies,
                                uint64_t *out_dev, size_t len_out, void *stream);
int pfhe_rand_seeded_expand(int device, const uint32_t *mask_key, const uint32_t *mask_nonce, size_t first_row,
                            size_t mask_len, size_t body_len, const uint64_t *bodies, size_t len_bodies, uint64_t *out,
                            size_t len_out);
int pfhe_rand32_uniform_dev(int device, const uint32_t *key, const uint32_t *nonce, size_t offset, uint32_t *out_dev, size_t n,
                            void *stream);
int pfhe_rand32_binary_dev(int device, const uint32_t *key, const uint32_t *nonce, size_t offset, uint32_t *out_dev, size_t n,
                           void *stream);
int pfhe_rand32_ternary_dev(int device, const uint32_t *key, const uint32_t *nonce, size_t offset, uint32_t *out_dev, size_t n,
                            void *stream);
int pfhe_rand32_tuniform_dev(int device, const uint32_t *key, const uint32_t *nonce, size_t offset, uint32_t bound_log2,
                             uint32_t *out_dev, size_t n, void *stream);
int pfhe_rand32_fill_rows_dev(int device, const uint32_t *mask_key, const uint32_t *mask_nonce, const uint32_t *noise_key,
                              const uint32_t *noise_nonce, size_t first_row, size_t mask_len, size_t body_len,
                              uint32_t bound_log2, int add, uint32_t *out_dev, size_t len_out, void *stream);
int pfhe_rand32_lwe_encrypt_seeded_dev(int device, const uint32_t *mask_key, const uint32_t *mask_nonce,
                                       const uint32_t *noise_key, const uint32_t *noise_nonce, size_t first_row,
                                       const uint32_t *lwe_key_dev, size_t dimension, uint32_t bound_log2, uint32_t *bodies_dev,
                                       size_t rows, void *stream);
int pfhe_rand32_lwe_encrypt_seeded(int device, const uint32_t *mask_key, const uint32_t *mask_nonce, const uint32_t *noise_key,
                                   const uint32_t *noise_nonce, size_t first_row, const uint32_t *lwe_key, size_t dimension,
                                   uint32_t bound_log2, uint32_t *bodies, size_t rows);
int pfhe_rand32_seeded_expand_dev(int device, const uint32_t *mask_key, const uint32_t *mask_nonce, size_t first_row,
                                  size_t mask_len, size_t body_len, const uint32_t *bodies_dev, size_t len_bodies,
                                  uint32_t *out_dev, size_t len_out, void *stream);
int pfhe_rand32_seeded_expand(int device, const uint32_t *mask_key, const uint32_t *mask_nonce, size_t first_row,
                              size_t mask_len, size_t body_len, const uint32_t *bodies, size_t len_bodies, uint32_t *out,
                              size_t len_out);

#ifdef __cplusplus
}
#endif
#endif /* PFHE_H */
