// pfhe_trace_device.hpp — what the kernels that apply a Galois automorphism share (pfhe_trace.hip, pfhe_ring_pack.hip): the
// exponents of a launch as a kernel argument, t^-1 modulo 2N, and one word of sigma_t(p).  DESIGN.md §21 states sigma_t.
#pragma once

#include "pfhe_tfhe_host.hpp"

namespace pfhe {

// the exponents of one launch sequence, as the kernels take them: step s applies sigma_{t[s]}; accumulate says whether a
// step adds its result to ACC (the trace) or replaces it (rule 1)
struct TraceSteps {
    u32 count, accumulate;
    u32 t[kMaxLogN];
};

// t^-1 modulo 2N (mask = 2N - 1) for odd t: t is its own inverse modulo 8, and each Newton step doubles the bits
__host__ __device__ inline u32 odd_inverse(u32 t, u32 mask) {
    u32 x = t;
#pragma unroll
    for (int i = 0; i < 4; ++i) x *= 2u - t * x;
    return x & mask;
}

// sigma_t(p)[i] of a polynomial of n words, t_inv = t^-1 mod 2n
template <class W>
__device__ __forceinline__ W sigma_word(const W *p, u32 i, u32 t_inv, u32 n) {
    const u32 u = (i * t_inv) & (2 * n - 1);
    const W v = p[u & (n - 1)];
    return (u & n) ? (W)0 - v : v;
}

}  // namespace pfhe
