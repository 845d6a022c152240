// The host side of primus-fhe_amd/csrc/pfhe_modmath.hpp (PFHE_HD functions) behind a C ABI, for tests/test_modmath_host.py:
// arrays in, arrays out, so that one call covers a whole table of operands.
#include <cstddef>
#include "pfhe_modmath.hpp"
using namespace pfhe;
extern "C" {
void shim_barrett_reduce128(const u64 *lo, const u64 *hi, size_t n, u64 q, u64 mu_lo, u64 mu_hi, u64 *out) {
    for (size_t i = 0; i < n; ++i) out[i] = barrett_reduce128(lo[i], hi[i], q, mu_lo, mu_hi);
}
void shim_mul_add_mod_barrett(const u64 *a, const u64 *b, const u64 *c, size_t n, u64 q, u64 mu_lo, u64 mu_hi, u64 *out) {
    for (size_t i = 0; i < n; ++i) out[i] = mul_add_mod_barrett(a[i], b[i], c[i], q, mu_lo, mu_hi);
}
void shim_mul_mod_barrett(const u64 *a, const u64 *b, size_t n, u64 q, u64 mu_lo, u64 mu_hi, u64 *out) {
    for (size_t i = 0; i < n; ++i) out[i] = mul_mod_barrett(a[i], b[i], q, mu_lo, mu_hi);
}
}
