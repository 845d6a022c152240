// Compile coverage of lwe_linear / lwe_linear_dev in include/pfhe.hpp, compiled only and never run: both function templates
// instantiated for both word types and both weight types.  tests/test_lwe_linear_cpu.py compares the pfhe_* symbols this
// unit leaves undefined with the 306 of cpp_mirror_symbols.txt plus cpp_mirror_linear_symbols.txt.
#include <cstdint>

#include "pfhe.hpp"

namespace pfhe {
#define PFHE_LINEAR_INSTANCES(W, S)                                                                                      \
    template void lwe_linear<W>(int, const W *, size_t, size_t, const S *, size_t, size_t, size_t, const W *, size_t, W *, \
                                size_t);                                                                                 \
    template void lwe_linear_dev<W>(int, const W *, size_t, size_t, const S *, size_t, size_t, size_t, const W *, size_t, \
                                    W *, size_t, void *);
PFHE_LINEAR_INSTANCES(uint64_t, uint64_t)
PFHE_LINEAR_INSTANCES(uint64_t, int8_t)
PFHE_LINEAR_INSTANCES(uint32_t, uint32_t)
PFHE_LINEAR_INSTANCES(uint32_t, int8_t)
#undef PFHE_LINEAR_INSTANCES
}  // namespace pfhe

// the weights' type picks the overload: a call with int8_t weights and one with words, deduced from the ciphertext
void every_overload_by_deduction(const uint32_t *in, const int8_t *w8, const uint32_t *w, uint32_t *out, void *stream) {
    pfhe::lwe_linear(0, in, 6, 1, w8, 3, 3, 1, nullptr, 0, out, 2);
    pfhe::lwe_linear(0, in, 6, 1, w, 3, 3, 1, nullptr, 0, out, 2);
    pfhe::lwe_linear_dev(0, in, 6, 1, w8, 3, 3, 1, nullptr, 0, out, 2, stream);
    pfhe::lwe_linear_dev(0, in, 6, 1, w, 3, 3, 1, nullptr, 0, out, 2);
}
