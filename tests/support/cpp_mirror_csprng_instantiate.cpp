// Compile coverage of the random layer of include/pfhe.hpp, compiled only and never run: every function template
// instantiated for both word types, and the one plain function called.  tests/test_csprng_cpu.py compares the pfhe_* symbols
// this unit leaves undefined with the 306 of cpp_mirror_symbols.txt plus cpp_mirror_csprng_symbols.txt.
#include <cstdint>

#include "pfhe.hpp"

namespace pfhe {
#define PFHE_RAND_INSTANCES(W)                                                                                             \
    template void torus_uniform_dev<W>(int, const RandSeed &, size_t, W *, size_t, void *);                                \
    template void torus_binary_dev<W>(int, const RandSeed &, size_t, W *, size_t, void *);                                 \
    template void torus_ternary_dev<W>(int, const RandSeed &, size_t, W *, size_t, void *);                                \
    template void torus_tuniform_dev<W>(int, const RandSeed &, size_t, uint32_t, W *, size_t, void *);                     \
    template void fill_rows_dev<W>(int, const RandSeed &, const RandSeed &, size_t, size_t, size_t, uint32_t, bool, W *,    \
                                   size_t, void *);                                                                        \
    template void lwe_encrypt_seeded<W>(int, const RandSeed &, const RandSeed &, size_t, const W *, size_t, uint32_t, W *, \
                                        size_t);                                                                           \
    template void lwe_encrypt_seeded_dev<W>(int, const RandSeed &, const RandSeed &, size_t, const W *, size_t, uint32_t,   \
                                            W *, size_t, void *);                                                          \
    template void seeded_expand<W>(int, const RandSeed &, size_t, size_t, size_t, const W *, size_t, W *, size_t);         \
    template void seeded_expand_dev<W>(int, const RandSeed &, size_t, size_t, size_t, const W *, size_t, W *, size_t, void *);
PFHE_RAND_INSTANCES(uint64_t)
PFHE_RAND_INSTANCES(uint32_t)
#undef PFHE_RAND_INSTANCES
}  // namespace pfhe

// the word is deduced from the first word pointer; a seed is built from eight key words and a 64-bit nonce
void every_call_by_deduction(const uint32_t (&key)[8], uint32_t *w32, uint64_t *w64, void *stream) {
    const pfhe::RandSeed mask(key, 1), noise(key, 0x8000000000000002ull);
    pfhe::csprng_keystream_dev(0, mask, 5, w32, 16, stream);
    pfhe::torus_uniform_dev(0, mask, 3, w64, 8);
    pfhe::torus_tuniform_dev(0, noise, 3, 17, w32, 8, stream);
    pfhe::fill_rows_dev(0, mask, noise, 0, 7, 1, 17, false, w64, 16);
    pfhe::lwe_encrypt_seeded_dev(0, mask, noise, 0, w32, 7, 17, w32 + 8, 2);
    pfhe::seeded_expand(0, mask, 0, 7, 1, w64, 2, w64 + 8, 16);
}
