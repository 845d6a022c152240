// pfhe_fft_device.hpp — device code of the torus FFT and of one fused TFHE external product (pfhe_fft.hip).
//
// The half-size transforms in LDS, the torus conversions, the signed digits, and the two halves of the fused product
// (k = 1, N <= 2^11): fused_accumulate_rows (digits, forward transforms and the multiply-accumulate of both input rows) and
// fused_inverse_rows (the two folded inverses and the torus wrap).  tfhe_fused_kernel runs them once on words read from
// global memory; tfhe_blindrot_loop_kernel and tfhe_bitrot_loop_kernel (pfhe_lut.hip) run them once per step on an
// accumulator that stays in LDS; so does tfhe_trace_loop_kernel (pfhe_trace.hip), on the mask row alone.  All inline the
// same code, so a step of a loop is the product's arithmetic, operation for operation.  RegisterRow (at the end of this
// file, with MonomialShift and rotated_diff) is the row of every form that holds its input row in registers.
// fused_accumulate_rows takes the key's Hermitian part from a key source: ClassicKey (one key in memory) or MultiBitKey
// (the multi-bit rotation's per-ciphertext combination of 2^g keys, mb_combined_slots, shared with the per-group and
// combined-key kernels).
#pragma once

#include "pfhe_common.hpp"

namespace pfhe {

constexpr int kFftThreads = 256;
constexpr u32 kFusedMaxLogN = 11;
constexpr int kFusedPer = (1 << (kFusedMaxLogN - 1)) / kFftThreads;  // half-spectrum slots per thread in the fused kernels

__device__ __forceinline__ u32 lpad(u32 i) { return i + (i >> 4); }
__host__ __device__ inline size_t lds_bytes(u32 log_n) {
    const u32 m = 1u << (log_n - 1);
    return (size_t)(m + (m >> 4) + 1) * sizeof(double2);
}
__device__ __forceinline__ u32 bitrev(u32 i, u32 log_m) { return log_m ? __brev(i) >> (32 - log_m) : 0u; }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

// forward, natural order in, bit-reversed out: spans M/2 .. 1, twiddle e^{-2 pi i j / 2h} after the difference
static __device__ void fft_dif(double2 *x, u32 log_m, u32 log_n, const double2 *__restrict__ tw) {
    const u32 half = (1u << log_m) >> 1;
    for (u32 lh = log_m; lh-- > 0;) {
        const u32 h = 1u << lh;
        for (u32 b = threadIdx.x; b < half; b += blockDim.x) {
            const u32 j = b & (h - 1);
            const u32 i0 = ((b >> lh) << (lh + 1)) + j, i1 = i0 + h;
            const double2 a = x[lpad(i0)], c = x[lpad(i1)];
            double2 w = tw[j << (log_n - lh)];
            w.y = -w.y;
            x[lpad(i0)] = cadd(a, c);
            x[lpad(i1)] = cmul(csub(a, c), w);
        }
        __syncthreads();
    }
}

// inverse (unscaled), bit-reversed in, natural out: spans 1 .. M/2, twiddle e^{+2 pi i j / 2h} before the sum
static __device__ void fft_dit(double2 *x, u32 log_m, u32 log_n, const double2 *__restrict__ tw) {
    const u32 half = (1u << log_m) >> 1;
    for (u32 lh = 0; lh < log_m; ++lh) {
        const u32 h = 1u << lh;
        for (u32 b = threadIdx.x; b < half; b += blockDim.x) {
            const u32 j = b & (h - 1);
            const u32 i0 = ((b >> lh) << (lh + 1)) + j, i1 = i0 + h;
            const double2 a = x[lpad(i0)], c = cmul(x[lpad(i1)], tw[j << (log_n - lh)]);
            x[lpad(i0)] = cadd(a, c);
            x[lpad(i1)] = csub(a, c);
        }
        __syncthreads();
    }
}

// TorusFftValue::into_f64_centered
__device__ __forceinline__ double centre(u32 x) { return (double)(int)x; }
__device__ __forceinline__ double centre(u64 x) { return (double)(long long)x; }

// TorusFftValue::from_f64_wrapping_rounded: round half away from zero, then `as i64 as u32` (saturating at +-2^63) or
// `as i128 as u64` (saturating at +-2^127, otherwise exact mod 2^64); NaN gives 0
template <class W>
__device__ __forceinline__ W to_torus(double v);
template <>
__device__ __forceinline__ u32 to_torus<u32>(double v) {
    const double r = round(v);
    if (r != r) return 0u;
    if (r >= 0x1p63) return 0xffffffffu;
    if (r <= -0x1p63) return 0u;
    return (u32)(u64)(long long)r;
}
template <>
__device__ __forceinline__ u64 to_torus<u64>(double v) {
    const double r = round(v);
    if (r != r) return 0ull;
    if (fabs(r) < 0x1p63) return (u64)(long long)r;
    if (r >= 0x1p127) return ~0ull;
    if (r <= -0x1p127) return 0ull;
    const u64 bits = (u64)__double_as_longlong(r);  // 2^63 <= |r| < 2^127: r = mant * 2^e, 11 <= e < 75
    const int e = (int)((bits >> 52) & 0x7ff) - 1075;
    const u64 mag = e >= 64 ? 0ull : ((bits & 0xfffffffffffffull) | (1ull << 52)) << e;
    return r < 0 ? 0ull - mag : mag;
}

// one OnceSignedDecomposer step (common.rs:219-274) on a power-of-two modulus: the digit as its centred f64 value
template <class W>
__device__ __forceinline__ double digit_step(W v, u32 shift, u32 log_basis, u32 &carry) {
    const W B = (W)1 << log_basis;
    const W temp = ((v >> shift) & (B - 1)) + (W)carry;
    const W cmask = log_basis == 1 ? (W)2 : (B | (B >> 1));
    const bool nc = (temp & cmask) != 0;
    carry = nc ? 1u : 0u;
    if (!nc) return (double)temp;
    return temp > B - 1 ? 0.0 : -(double)(B - temp);  // temp + (2^BITS - B), reinterpreted as signed
}
template <class W>
__device__ __forceinline__ u32 init_carry(W v, u32 drop_bits) {
    return drop_bits ? (u32)((v >> (drop_bits - 1)) & 1) : 0u;
}
// One signed digit of v as a word modulo 2^BITS, for the key switches that multiply digits as integers; levels are walked
// least significant first, from carry = init_carry(v, drop_bits).  digit_step is the rule and is called for the carry it
// decides only: the digit as a word is field + carry_in - carry_out * B, which is digit_step's value for any log_basis.
template <class W>
__device__ __forceinline__ W digit_word(W v, u32 shift, u32 log_basis, u32 &carry) {
    const W field = (v >> shift) & (((W)1 << log_basis) - 1);
    const W carry_in = (W)carry;
    (void)digit_step(v, shift, log_basis, carry);
    return field + carry_in - ((W)carry << log_basis);
}

struct Shape {
    u32 log_n, k, log_basis, ell, drop_bits;
};

// ---------------- the multi-bit key combination ----------------
//
// A group of g mask elements has 2^g keys, key j for the pattern j of the group's key bits.  With r_j the sum of the
// group's exponents at the set bits of j (modulo 2N), the per-ciphertext key is K = sum_j X^{r_j} K_j; the product sees
// only its Hermitian part, and the spectrum M(r) of X^r is Hermitian-symmetric, so the arithmetic is DEFINED on
// half-spectrum slots: Kh[m] = sum_j M(r_j)[2m] Herm(K_j)[2m], M(r)[k'] = root[(r (1 - 2k')) mod 2N], root[i] = tw[i] for
// i < N and -tw[i - N] otherwise.  j ascending, the j = 0 term added without a multiplication, every multiply-add an
// explicit fma: the same bits in every kernel that inlines mb_combined_slots.

// Herm(K)[2i] of one key polynomial in the reference's layout, as fused_accumulate_rows' classic source forms it
__device__ __forceinline__ double2 herm_slot(const double2 *__restrict__ kp, u32 i, u32 n) {
    const double2 a = kp[2 * i], b = kp[(n + 1 - 2 * i) & (n - 1)];
    return make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
}

// the exponents of one group of one ciphertext, each modulo 2N; 0 past the grouping factor
struct MbExps {
    u32 e0, e1, e2, e3;
};
__device__ __forceinline__ MbExps mb_load_exps(const u32 *__restrict__ ex, u32 g, u32 n) {
    const u32 mask = 2 * n - 1;
    return MbExps{ex[0] & mask, g > 1 ? ex[1] & mask : 0u, g > 2 ? ex[2] & mask : 0u, g > 3 ? ex[3] & mask : 0u};
}

// kh[c] = Kh[i] of C key polynomials that share the slot: herm(j, c) is Herm(K_j)[2i] of polynomial c.  The twiddle index
// stays in 32 bits: r < 2N <= 2^15 and 4i < 2N, so r 4i < 2^30, and wrapping modulo 2^32 agrees with modulo 2N.
template <int C, class Herm>
__device__ __forceinline__ void mb_combined_slots(const Herm herm, const MbExps x, u32 g, u32 i, u32 n,
                                                  const double2 *__restrict__ tw, double2 (&kh)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) kh[c] = herm(0u, c);
    for (u32 j = 1; j < (1u << g); ++j) {
        const u32 r = ((j & 1 ? x.e0 : 0u) + (j & 2 ? x.e1 : 0u) + (j & 4 ? x.e2 : 0u) + (j & 8 ? x.e3 : 0u)) & (2 * n - 1);
        const u32 idx = (r - r * 4 * i) & (2 * n - 1);
        double2 w = tw[idx & (n - 1)];
        if (idx & n) w = make_double2(-w.x, -w.y);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double2 h = herm(j, c);
            kh[c].x = fma(-w.y, h.y, fma(w.x, h.x, kh[c].x));
            kh[c].y = fma(w.y, h.x, fma(w.x, h.y, kh[c].y));
        }
    }
}

// acc + d * h in ONE fixed sequence of operations, whatever surrounds the call: the two cross products rounded on their own,
// the other two fused, then the adds.  Every multiply-accumulate of a digit spectrum with a key's Hermitian part goes
// through here, the classic product's and the multi-bit rotation's alike, so all of them round alike.  Left to contraction
// the pairing depends on where h comes from (loaded or averaged from memory: this one; out of a chain of fused
// multiply-adds: the other pairing of the imaginary part), and the forms would differ in the last bit.
__device__ __forceinline__ double2 cmac_fixed(double2 acc, double2 d, double2 h) {
#pragma clang fp contract(off)
    const double x = fma(d.x, h.x, -(d.y * h.y));
    const double y = fma(d.y, h.x, d.x * h.y);
    return make_double2(acc.x + x, acc.y + y);
}

// the multi-bit key source of fused_accumulate_rows: the group's 2^g keys end to end in the reference's layout
struct MultiBitKey {
    const double2 *__restrict__ keys;
    u64 key_len;
    MbExps x;
    u32 g;
    struct Level {
        const double2 *k0;
        u64 key_len;
        MbExps x;
        u32 g, n;
        __device__ __forceinline__ void mac(u32 i, const double2 *__restrict__ tw, double2 d, double2 &acc0,
                                            double2 &acc1) const {
            double2 kh[2];
            mb_combined_slots<2>([&](u32 j, int c) { return herm_slot(k0 + j * key_len + (u32)c * n, i, n); }, x, g, i, n, tw, kh);
            acc0 = cmac_fixed(acc0, d, kh[0]);
            acc1 = cmac_fixed(acc1, d, kh[1]);
        }
    };
    __device__ __forceinline__ Level level(u32 rl, u32 n) const { return Level{keys + (u64)(rl * 2) * n, key_len, x, g, n}; }
};

// ---------------- the fused product (k = 1, N <= 2^11), one workgroup per ciphertext ----------------
//
// Thread t owns coefficient pairs (i, i + N/2) and half-spectrum slots i for i = t + 256 u; the accumulators of both
// output rows stay in its registers.  The key is read in natural order (even entries and their mirrored odd partners),
// the digit spectrum from LDS at the bit-reversed position.

// input row r of a ciphertext in global memory: the words are re-read at every level (L1 hits)
template <class W>
struct GlobalRow {
    const W *xr;
    u32 m;
    __device__ __forceinline__ W lo(int, u32 i) const { return xr[i]; }
    __device__ __forceinline__ W hi(int, u32 i) const { return xr[i + m]; }
};

// Where the Hermitian part of the key comes from.  level(rl, n) fixes the key polynomials of input row r and level l
// (rl = r ell + l); mac(i, tw, d, acc0, acc1) adds d * Herm(key[r][l][0 / 1])[2i] to the two accumulators.  The classic
// source reads ONE key in the reference's layout.
struct ClassicKey {
    const double2 *__restrict__ key;
    struct Level {
        const double2 *k0, *k1;
        u32 n;
        __device__ __forceinline__ void mac(u32 i, const double2 *, double2 d, double2 &acc0, double2 &acc1) const {
            const u32 j = (n + 1 - 2 * i) & (n - 1);
            const double2 a0 = k0[2 * i], b0 = k0[j], a1 = k1[2 * i], b1 = k1[j];
            acc0 = cmac_fixed(acc0, d, make_double2(0.5 * (a0.x + b0.x), 0.5 * (a0.y - b0.y)));
            acc1 = cmac_fixed(acc1, d, make_double2(0.5 * (a1.x + b1.x), 0.5 * (a1.y - b1.y)));
        }
    };
    __device__ __forceinline__ Level level(u32 rl, u32 n) const {
        const double2 *k0 = key + (u64)(rl * 2) * n;
        return Level{k0, k0 + n, n};
    }
};

// both input rows, all levels: rows(r) gives row r, whose lo(u, i) / hi(u, i) are the words of coefficients i and
// i + N/2 of slot u.  Per level: their signed digits, the forward half transform in lds_p, and acc0 / acc1 += spectrum *
// Herm(key[r][l][0 / 1]) as the key source gives it.  Only the carries stay in registers between levels: bit u of carry0 / carry1 is the carry of
// coefficient i / i + N/2 of slot u.  Ends behind a barrier.  ROWS = 1 walks the mask row alone, against a key of ell
// rows (the key switch of pfhe_trace.hip): the same code, one trip of the outer loop.
template <class W, u32 ROWS = 2, class Rows, class Key>
__device__ __forceinline__ void fused_accumulate_rows(const Rows rows, const Key key, double2 *lds_p,
                                                      const double2 *__restrict__ tw, const Shape s,
                                                      double2 (&acc0)[kFusedPer], double2 (&acc1)[kFusedPer]) {
    const u32 n = 1u << s.log_n, m = n >> 1, log_m = s.log_n - 1;
    for (u32 r = 0; r < ROWS; ++r) {
        const auto row = rows(r);
        u32 carry0 = 0, carry1 = 0;
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) {
            const u32 i = threadIdx.x + u * kFftThreads;
            if (i < m) {
                carry0 |= init_carry(row.lo(u, i), s.drop_bits) << u;
                carry1 |= init_carry(row.hi(u, i), s.drop_bits) << u;
            }
        }
        for (u32 l = 0; l < s.ell; ++l) {
            const u32 shift = s.drop_bits + l * s.log_basis;
#pragma unroll
            for (int u = 0; u < kFusedPer; ++u) {
                const u32 i = threadIdx.x + u * kFftThreads;
                if (i < m) {
                    u32 c0 = (carry0 >> u) & 1, c1 = (carry1 >> u) & 1;
                    const double d0 = digit_step(row.lo(u, i), shift, s.log_basis, c0);
                    const double d1 = digit_step(row.hi(u, i), shift, s.log_basis, c1);
                    carry0 = (carry0 & ~(1u << u)) | (c0 << u);
                    carry1 = (carry1 & ~(1u << u)) | (c1 << u);
                    lds_p[lpad(i)] = cmul(make_double2(d0, d1), tw[i]);
                }
            }
            __syncthreads();
            fft_dif(lds_p, log_m, s.log_n, tw);
            const auto kl = key.level(r * s.ell + l, n);
#pragma unroll
            for (int u = 0; u < kFusedPer; ++u) {
                const u32 i = threadIdx.x + u * kFftThreads;
                if (i < m) {
                    const double2 d = lds_p[lpad(bitrev(i, log_m))];
                    kl.mac(i, tw, d, acc0[u], acc1[u]);
                }
            }
            __syncthreads();  // the next level overwrites the digit spectrum
        }
    }
}

// the two folded inverses of acc0 / acc1: sink(c, i, value of coefficient i, value of coefficient i + N/2) for output row
// c takes the scaled f64 values and wraps them to the torus (to_torus).  Ends behind a barrier.
template <class Sink>
__device__ __forceinline__ void fused_inverse_rows(const double2 (&acc0)[kFusedPer], const double2 (&acc1)[kFusedPer],
                                                   double2 *lds_p, const double2 *__restrict__ tw, const Shape s,
                                                   const Sink sink) {
    const u32 n = 1u << s.log_n, m = n >> 1, log_m = s.log_n - 1;
    const double scale = 1.0 / (double)m;
#pragma unroll
    for (u32 c = 0; c < 2; ++c) {
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) {
            const u32 i = threadIdx.x + u * kFftThreads;
            if (i < m) lds_p[lpad(bitrev(i, log_m))] = c ? acc1[u] : acc0[u];
        }
        __syncthreads();
        fft_dit(lds_p, log_m, s.log_n, tw);
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) {
            const u32 i = threadIdx.x + u * kFftThreads;
            if (i < m) {
                const double2 t = tw[i];
                const double2 v = cmul(lds_p[lpad(i)], make_double2(t.x, -t.y));
                sink(c, i, v.x * scale, v.y * scale);
            }
        }
        __syncthreads();  // the second row reuses the buffer
    }
}

// ---------------- the rows of a rotation step, held in registers ----------------

// X^r p for a polynomial p of N words, r taken modulo 2N: coefficient j is +-p[(j - r) mod N], the wrapped part negated;
// r >= N (high, rot = r - N) negates the other part
struct MonomialShift {
    u32 n, rot;
    bool high;
    __device__ __forceinline__ MonomialShift(u32 r, u32 n) : n(n) {
        r &= 2 * n - 1;
        high = r >= n;
        rot = high ? r - n : r;
    }
    // the index of the word that coefficient j takes ...
    __device__ __forceinline__ u32 source(u32 j) const { return (j - rot) & (n - 1); }
    // ... and that word, v, with coefficient j's sign
    template <class W>
    __device__ __forceinline__ W apply(u32 j, W v) const {
        return ((j < rot) != high) ? (W)0 - v : v;
    }
};

// coefficient j of X^r * p - p for a polynomial p of N words (wrapping arithmetic)
template <class W>
__device__ __forceinline__ W rotated_diff(const W *p, u32 j, const MonomialShift &x) {
    return x.apply(j, p[x.source(j)]) - p[j];
}

// one input row formed once and held in registers for all its levels: slot u holds coefficients i and i + N/2, i = thread +
// 256 u.  A row of X^r ACC - ACC here, of d1 - d0 in pfhe_cmux.hip, of sigma_t(ACC) in pfhe_trace.hip.
template <class W>
struct RegisterRow {
    W a[kFusedPer], b[kFusedPer];
    __device__ __forceinline__ W lo(int u, u32) const { return a[u]; }
    __device__ __forceinline__ W hi(int u, u32) const { return b[u]; }
};

}  // namespace pfhe
