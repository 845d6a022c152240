// pfhe_fft.hip — torus FFT tables (FullComplex64FftTable) and the TFHE external product in the Fourier domain
// (primus_fft, primus_lattice::tfhe).  include/pfhe.h: pfhe_fft_*, pfhe_tfhe_*, pfhe_tfhe32_*.
//
// Every transform runs at N/2 complex points.  For real x and Y = FFT_N(x_j psi^j), psi = e^{i pi/N}:
//   Y[(1 - k) mod N] = conj(Y[k])                                       (the odd entries are redundant)
//   Y[2m] = FFT_{N/2}((x_m + i x_{m+N/2}) e^{i pi m/N}),  m < N/2       (the folded negacyclic transform)
// The reference's inverse takes Re of the full inverse, which equals the folded inverse of the Hermitian part
// H[2m] = (Y[2m] + conj(Y[(1 - 2m) mod N])) / 2 on any spectrum; the standalone inverse forms H from both entries.
//
// One workgroup per polynomial, the N/2-point transform in LDS: a radix-2 decimation-in-frequency forward (natural in,
// bit-reversed out) and a decimation-in-time inverse (bit-reversed in, natural out), so no permutation pass is needed.
// LDS index i is stored at i + i/16 (one 16-byte slot of padding per 16) to spread the power-of-two strides over banks.
// Twiddles are the host's cis(pi j / N), j < N (complex64/table.rs:76-81, one rounding of the angle): the butterfly of
// span h uses e^{-+2 pi i j / 2h} = cis(-+pi (j N/h) / N).
//
// The external product (tfhe/external_product.rs:36-93): per input row r and level l, the signed digits of
// init_carry_slice + decompose_iter (decompose/primitive/basis.rs, common.rs) go through a forward half transform and
// are multiplied into k+1 half-spectrum accumulators with the key's Hermitian part (K[2m] + conj(K[(1-2m) mod N])) / 2 —
// the digits are real, so Re(ifft(D K)) = ifft(D Herm(K)) for any key — then k+1 folded inverses and the torus wrap.
//   fused   (k = 1, N <= 2^11): one launch, a workgroup per ciphertext; digits, digit spectrum and accumulators on chip
//            (accumulators in registers), the key read from L2;
//   general (every other shape): key Hermitian part, digit transforms, one multiply-accumulate kernel and the batched
//            inverse over plan-owned scratch.
// Summation order is fixed (rows, then levels); no atomics: results do not depend on batch size or chunking.
//
// The blind rotation over the product (pfhe_tfhe{,32}_blindrot_*): per step and ciphertext, ACC += (X^r ACC - ACC) (x) BSK_i.
//   whole loop (the fused shape): one launch per chunk, a workgroup per ciphertext, ACC in LDS from the first step to the
//            last, the fused product's own device code per step;
//   per step  (every other shape, or PFHE_DISABLE_FUSED_TFHE_BLINDROT): the product's launches plus one glue launch.
//
// The multi-bit rotation (pfhe_tfhe{,32}_mbrot_*, pfhe_tfhe_mb_combine_key_dev): per group of g mask elements and ciphertext,
// ACC = ACC (x) sum_j X^{r_j} BSK[t][j], the per-ciphertext key formed slot by slot in the Fourier domain (mb_combined_slots).
//   whole loop (the fused shape): one launch per chunk, ACC in LDS across all groups, the key formed inside the accumulate code;
//   per group  (every other shape, or the same switch): the Hermitian parts of the group's 2^g keys, the digit transforms of
//            ACC, a multiply-accumulate that forms the key per ciphertext, the inverses back into ACC;
//   combined key as a call of its own: one ciphertext's key of one group in the reference's layout, for the plain product.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <memory>
#include <type_traits>
#include <vector>

#include "pfhe_fft_device.hpp"
#include "pfhe_tfhe_exact_device.hpp"
#include "pfhe_tfhe_handles.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// ---------------- standalone batched transforms ----------------

// forward_torus_slice: count polynomials of N words -> count x N complex (the reference's full layout)
template <class W>
__global__ __launch_bounds__(kThreads) void fft_forward_kernel(const W *__restrict__ in, double2 *__restrict__ out,
                                                               const double2 *__restrict__ tw, u32 log_n) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_f[];
    const u32 n = 1u << log_n, m = n >> 1, log_m = log_n - 1;
    const W *x = in + (size_t)blockIdx.x * n;
    double2 *y = out + (size_t)blockIdx.x * n;
    for (u32 i = threadIdx.x; i < m; i += blockDim.x)
        lds_f[lpad(i)] = cmul(make_double2(centre(x[i]), centre(x[i + m])), tw[i]);
    __syncthreads();
    fft_dif(lds_f, log_m, log_n, tw);
    for (u32 i = threadIdx.x; i < m; i += blockDim.x) {
        const double2 v = lds_f[lpad(bitrev(i, log_m))];
        y[2 * i] = v;
        y[(n + 1 - 2 * i) & (n - 1)] = make_double2(v.x, -v.y);
    }
}

// inverse_torus_slice (FULL: count x N complex in the reference's layout, Hermitian part formed here) or the
// product's accumulators (!FULL: count x N/2 half-spectrum values, natural order)
template <class W, bool FULL>
__global__ __launch_bounds__(kThreads) void fft_inverse_kernel(const double2 *__restrict__ in, W *__restrict__ out,
                                                               const double2 *__restrict__ tw, u32 log_n) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_i[];
    const u32 n = 1u << log_n, m = n >> 1, log_m = log_n - 1;
    W *x = out + (size_t)blockIdx.x * n;
    if constexpr (FULL) {
        const double2 *y = in + (size_t)blockIdx.x * n;
        for (u32 i = threadIdx.x; i < m; i += blockDim.x) {
            const double2 a = y[2 * i], b = y[(n + 1 - 2 * i) & (n - 1)];
            lds_i[lpad(bitrev(i, log_m))] = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
        }
    } else {
        const double2 *y = in + (size_t)blockIdx.x * m;
        for (u32 i = threadIdx.x; i < m; i += blockDim.x) lds_i[lpad(bitrev(i, log_m))] = y[i];
    }
    __syncthreads();
    fft_dit(lds_i, log_m, log_n, tw);
    const double scale = 1.0 / (double)m;  // exact: a power of two
    for (u32 i = threadIdx.x; i < m; i += blockDim.x) {
        const double2 t = tw[i];
        const double2 v = cmul(lds_i[lpad(i)], make_double2(t.x, -t.y));
        x[i] = to_torus<W>(v.x * scale);
        x[i + m] = to_torus<W>(v.y * scale);
    }
}

// ---------------- the general product ----------------

// the key's Hermitian part, natural order: keyh[p][i] = (K[p][2i] + conj(K[p][(1 - 2i) mod N])) / 2
__global__ __launch_bounds__(kThreads) void tfhe_key_herm_kernel(const double2 *__restrict__ key, double2 *__restrict__ keyh,
                                                                 u32 log_n, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n, m = n >> 1;
    const u64 p = t >> (log_n - 1);
    const u32 i = (u32)(t & (m - 1));
    const double2 a = key[p * n + 2 * i], b = key[p * n + ((n + 1 - 2 * i) & (n - 1))];
    keyh[t] = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
}

// one workgroup per digit polynomial (ciphertext e, row r, level l): its digits (the carry chain from level 0), the
// forward half transform, written in natural order to spec[((e (k+1) + r) ell + l) N/2 + i]
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_digit_fwd_kernel(const W *__restrict__ in, double2 *__restrict__ spec,
                                                                  const double2 *__restrict__ tw, Shape s) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_d[];
    const u32 n = 1u << s.log_n, m = n >> 1, log_m = s.log_n - 1;
    const u32 lvl = blockIdx.x % s.ell;
    const u64 poly = blockIdx.x / s.ell;  // e * (k+1) + r
    const W *x = in + poly * n;
    for (u32 i = threadIdx.x; i < m; i += blockDim.x) {
        const W v0 = x[i], v1 = x[i + m];
        u32 c0 = init_carry(v0, s.drop_bits), c1 = init_carry(v1, s.drop_bits);
        double d0 = 0.0, d1 = 0.0;
        for (u32 l = 0; l <= lvl; ++l) {
            const u32 shift = s.drop_bits + l * s.log_basis;
            d0 = digit_step(v0, shift, s.log_basis, c0);
            d1 = digit_step(v1, shift, s.log_basis, c1);
        }
        lds_d[lpad(i)] = cmul(make_double2(d0, d1), tw[i]);
    }
    __syncthreads();
    fft_dif(lds_d, log_m, s.log_n, tw);
    double2 *out = spec + (u64)blockIdx.x * m;
    for (u32 i = threadIdx.x; i < m; i += blockDim.x) out[i] = lds_d[lpad(bitrev(i, log_m))];
}

// acc[e][c][i] = sum over r < in_rows, l (in that order) of spec[e][r][l][i] * keyh[r][l][c][i], c <= k.  The product
// decomposes all k+1 rows of its input; the trace (pfhe_trace.hip) the k mask rows alone, against a key of k ell rows.
__global__ __launch_bounds__(kThreads) void tfhe_mulacc_kernel(const double2 *__restrict__ spec,
                                                               const double2 *__restrict__ keyh, double2 *__restrict__ acc,
                                                               u32 log_n, u32 k, u32 ell, u32 in_rows, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 m = 1u << (log_n - 1), cols = k + 1;
    const u32 i = (u32)(t & (m - 1));
    const u64 ec = t >> (log_n - 1);
    const u32 c = (u32)(ec % cols);
    const u64 e = ec / cols;
    const double2 *sp = spec + e * in_rows * ell * m + i;
    const double2 *kh = keyh + (u64)c * m + i;
    double2 a = make_double2(0.0, 0.0);
    for (u32 rl = 0; rl < in_rows * ell; ++rl) a = cmac_fixed(a, sp[(u64)rl * m], kh[(u64)rl * cols * m]);
    acc[t] = a;
}

// ---------------- the fused product (k = 1, N <= 2^11) ----------------

// one workgroup per ciphertext; the body is pfhe_fft_device.hpp's fused_accumulate_rows / fused_inverse_rows
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_fused_kernel(const W *__restrict__ in, const double2 *__restrict__ key,
                                                              W *__restrict__ out, const double2 *__restrict__ tw, Shape s) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_p[];
    const u32 n = 1u << s.log_n, m = n >> 1;
    const W *x = in + (u64)blockIdx.x * 2 * n;
    W *o = out + (u64)blockIdx.x * 2 * n;
    double2 acc0[kFusedPer], acc1[kFusedPer];
#pragma unroll
    for (int u = 0; u < kFusedPer; ++u) acc0[u] = acc1[u] = make_double2(0.0, 0.0);
    fused_accumulate_rows<W>([&](u32 r) { return GlobalRow<W>{x + r * n, m}; }, ClassicKey{key}, lds_p, tw, s, acc0, acc1);
    fused_inverse_rows(acc0, acc1, lds_p, tw, s, [&](u32 c, u32 i, double lo, double hi) {
        o[c * n + i] = to_torus<W>(lo);
        o[c * n + i + m] = to_torus<W>(hi);
    });
}

// ---------------- blind rotation over the product ----------------

// The whole loop of one ciphertext in one workgroup (k = 1, N <= 2^11): ACC (2N words) sits in LDS behind the digit
// spectrum from the first step to the last.  Per step: D row by row from the LDS-resident ACC into registers, the
// product's own accumulate and inverse code against step i's key (global memory, natural order), ACC += E in LDS.  Every
// gather of a step precedes a barrier of fused_accumulate_rows, every update follows them, and fused_inverse_rows
// ends behind a barrier, so no step reads a word the same step has already updated.
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_blindrot_loop_kernel(W *__restrict__ acc, const double2 *__restrict__ bsk,
                                                                      const u32 *__restrict__ exps, u32 n_steps,
                                                                      const double2 *__restrict__ tw, Shape s) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_l[];
    const u32 n = 1u << s.log_n, m = n >> 1;
    W *a = reinterpret_cast<W *>(reinterpret_cast<char *>(lds_l) + lds_bytes(s.log_n));
    W *g = acc + (u64)blockIdx.x * 2 * n;
    for (u32 i = threadIdx.x; i < 2 * n; i += blockDim.x) a[i] = g[i];
    __syncthreads();
    const u32 *ex = exps + (u64)blockIdx.x * n_steps;
    const u64 key_len = (u64)4 * s.ell * n;
    for (u32 step = 0; step < n_steps; ++step) {
        const MonomialShift x(ex[step], n);  // the device form takes every exponent modulo 2N
        const double2 *key = bsk + step * key_len;
        double2 acc0[kFusedPer], acc1[kFusedPer];
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) acc0[u] = acc1[u] = make_double2(0.0, 0.0);
        fused_accumulate_rows<W>([&](u32 row) {
            RegisterRow<W> d;
#pragma unroll
            for (int u = 0; u < kFusedPer; ++u) {
                const u32 i = threadIdx.x + u * kThreads;
                d.a[u] = i < m ? rotated_diff(a + row * n, i, x) : (W)0;
                d.b[u] = i < m ? rotated_diff(a + row * n, i + m, x) : (W)0;
            }
            return d;
        }, ClassicKey{key}, lds_l, tw, s, acc0, acc1);
        fused_inverse_rows(acc0, acc1, lds_l, tw, s, [&](u32 c, u32 i, double lo, double hi) {
            a[c * n + i] += to_torus<W>(lo);
            a[c * n + i + m] += to_torus<W>(hi);
        });
    }
    for (u32 i = threadIdx.x; i < 2 * n; i += blockDim.x) g[i] = a[i];
}

// ---------------- the multi-bit blind rotation ----------------

// input row r of an accumulator that sits in LDS: read in place at every level, no rotated difference is formed
template <class W>
struct LdsRow {
    const W *xr;
    u32 m;
    __device__ __forceinline__ W lo(int, u32 i) const { return xr[i]; }
    __device__ __forceinline__ W hi(int, u32 i) const { return xr[i + m]; }
};

// The whole multi-bit loop of one ciphertext in one workgroup (k = 1, N <= 2^11), ACC in LDS behind the digit spectrum as
// in tfhe_blindrot_loop_kernel.  Per group of g mask elements: ACC = ACC (x) K with K = sum_j X^{r_j} BSK[t][j] formed slot
// by slot in the accumulate code (MultiBitKey), the sink ASSIGNS to_torus(E) to ACC.  Every read of ACC in a group precedes
// the barrier that ends fused_accumulate_rows, every write follows it, and fused_inverse_rows ends behind a barrier.
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_mb_blindrot_loop_kernel(W *__restrict__ acc, const double2 *__restrict__ bsk,
                                                                         const u32 *__restrict__ exps, u32 groups, u32 g,
                                                                         const double2 *__restrict__ tw, Shape s) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_m[];
    const u32 n = 1u << s.log_n, m = n >> 1;
    W *a = reinterpret_cast<W *>(reinterpret_cast<char *>(lds_m) + lds_bytes(s.log_n));
    W *gl = acc + (u64)blockIdx.x * 2 * n;
    for (u32 i = threadIdx.x; i < 2 * n; i += blockDim.x) a[i] = gl[i];
    __syncthreads();
    const u32 *ex = exps + (u64)blockIdx.x * groups * g;
    const u64 key_len = (u64)4 * s.ell * n;
    for (u32 t = 0; t < groups; ++t) {
        const MultiBitKey key{bsk + ((u64)t << g) * key_len, key_len, mb_load_exps(ex + t * g, g, n), g};
        double2 acc0[kFusedPer], acc1[kFusedPer];
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) acc0[u] = acc1[u] = make_double2(0.0, 0.0);
        fused_accumulate_rows<W>([&](u32 row) { return LdsRow<W>{a + row * n, m}; }, key, lds_m, tw, s, acc0, acc1);
        fused_inverse_rows(acc0, acc1, lds_m, tw, s, [&](u32 c, u32 i, double lo, double hi) {
            a[c * n + i] = to_torus<W>(lo);
            a[c * n + i + m] = to_torus<W>(hi);
        });
    }
    for (u32 i = threadIdx.x; i < 2 * n; i += blockDim.x) gl[i] = a[i];
}

// tfhe_mulacc_kernel with the key's Hermitian part formed per ciphertext: keyh holds the Hermitian parts of the group's 2^g
// keys (tfhe_key_herm_kernel's output, key after key), exps points at the group's first exponent of ciphertext 0 and
// ciphertext e's are exp_stride further on.  acc[e][c][i] = sum over r, l (in that order) of spec[e][r][l][i] * Kh_e[r][l][c][i]
__global__ __launch_bounds__(kThreads) void tfhe_mb_mulacc_kernel(const double2 *__restrict__ spec,
                                                                  const double2 *__restrict__ keyh, double2 *__restrict__ acc,
                                                                  const u32 *__restrict__ exps, u32 exp_stride, u32 g,
                                                                  const double2 *__restrict__ tw, u32 log_n, u32 k, u32 ell,
                                                                  u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n, m = n >> 1, rows = k + 1;
    const u32 i = (u32)(t & (m - 1));
    const u64 ec = t >> (log_n - 1);
    const u32 c = (u32)(ec % rows);
    const u64 e = ec / rows;
    const MbExps x = mb_load_exps(exps + e * exp_stride, g, n);
    const double2 *sp = spec + e * rows * ell * m + i;
    const double2 *kh = keyh + (u64)c * m + i;
    const u64 keyh_len = (u64)rows * ell * rows * m;
    double2 a = make_double2(0.0, 0.0);
    for (u32 rl = 0; rl < rows * ell; ++rl) {
        double2 kc[1];
        mb_combined_slots<1>([&](u32 j, int) { return kh[j * keyh_len + (u64)rl * rows * m]; }, x, g, i, n, tw, kc);
        a = cmac_fixed(a, sp[(u64)rl * m], kc[0]);
    }
    acc[t] = a;
}

// The combined key of ONE ciphertext and ONE group as a key of its own, in the reference's full layout: for polynomial p
// and slot i, out[p][2i] = Kh[i] and out[p][(1 - 2i) mod N] = conj(Kh[i]).  The product's Hermitian step returns Kh[i] from
// that bit for bit ((x + x) * 0.5 is exact).
__global__ __launch_bounds__(kThreads) void tfhe_mb_combine_key_kernel(const double2 *__restrict__ keys,
                                                                       const u32 *__restrict__ exps, double2 *__restrict__ out,
                                                                       u32 g, const double2 *__restrict__ tw, u32 log_n,
                                                                       u64 key_len, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n, m = n >> 1;
    const u64 p = t >> (log_n - 1);
    const u32 i = (u32)(t & (m - 1));
    double2 kc[1];
    mb_combined_slots<1>([&](u32 j, int) { return herm_slot(keys + j * key_len + p * n, i, n); }, mb_load_exps(exps, g, n), g, i,
                         n, tw, kc);
    out[p * n + 2 * i] = kc[0];
    out[p * n + ((n + 1 - 2 * i) & (n - 1))] = make_double2(kc[0].x, -kc[0].y);
}

// The element-wise glue of the per-step form, one thread per coefficient, as blindrot_glue_kernel on torus words:
// ACC' = ACC + E (ADD_E; stored when STORE_ACC) and D' = X^r ACC' - ACC' (ROT == kRotSub) or X^r ACC' alone (kRotOnly).
// The rotated source word is gathered as ACC + E at that index, so ACC' goes to another buffer than it is read from.
// Coefficient i belongs to polynomial p = i >> log_n of element p / polys_per_exp, which takes exps[element * exp_stride].
enum TorusRot : int { kRotNone = 0, kRotSub = 1, kRotOnly = 2 };

template <class W, bool ADD_E, bool STORE_ACC, int ROT>
__global__ __launch_bounds__(kThreads) void tfhe_blindrot_glue_kernel(const W *__restrict__ acc, const W *__restrict__ e_in,
                                                                      W *__restrict__ acc_out, W *__restrict__ d_out,
                                                                      const u32 *__restrict__ exps, u32 exp_stride,
                                                                      u32 polys_per_exp, u32 log_n, u64 total) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const u32 n = 1u << log_n, mask = n - 1;
    const W a = ADD_E ? (W)(acc[i] + e_in[i]) : acc[i];
    if constexpr (STORE_ACC) acc_out[i] = a;
    if constexpr (ROT != kRotNone) {
        const u64 el = (i >> log_n) / polys_per_exp;
        const MonomialShift shift(exps[el * exp_stride], n);
        const u32 j = (u32)(i & mask);
        const u64 src = (i - j) + shift.source(j);
        const W x = shift.apply(j, ADD_E ? (W)(acc[src] + e_in[src]) : acc[src]);
        d_out[i] = ROT == kRotSub ? (W)(x - a) : x;
    }
}

}  // namespace
}  // namespace pfhe

namespace {

// kernels with more than 64 KiB of LDS need the attribute once per device (pfhe_fft_create sets it)
template <class W>
int set_lds_attributes(size_t bytes) {
    if (bytes <= 64 * 1024) return PFHE_OK;
    const void *kerns[] = {reinterpret_cast<const void *>(fft_forward_kernel<W>),
                           reinterpret_cast<const void *>(fft_inverse_kernel<W, true>),
                           reinterpret_cast<const void *>(fft_inverse_kernel<W, false>),
                           reinterpret_cast<const void *>(tfhe_digit_fwd_kernel<W>)};
    for (const void *k : kerns) PFHE_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return PFHE_OK;
}

template <class W>
int forward_dev(const pfhe_fft *f, const W *in, size_t len_in, double *out, size_t len_out, hipStream_t s) {
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    if (len_in % f->n != 0 || len_out != len_in) {
        set_last_error("fft forward: input must be count*N words and output count*N complex values");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_in == 0) return PFHE_OK;
    if (!in || !out) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(in);
    PFHE_REQUIRE_ALIGNED(out);
    const u64 count = len_in / f->n;
    if (count > 0x7fffffffull) return PFHE_ERR_BAD_LENGTH;
    DeviceGuard g(f->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return launch_groups(fft_forward_kernel<W>, count, lds_bytes(f->log_n), s, in, (double2 *)out, f->tw, f->log_n);
}

template <class W>
int inverse_dev(const pfhe_fft *f, const double *in, size_t len_in, W *out, size_t len_out, hipStream_t s) {
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    if (len_in % f->n != 0 || len_out != len_in) {
        set_last_error("fft inverse: input must be count*N complex values and output count*N words");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_in == 0) return PFHE_OK;
    if (!in || !out) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(in);
    PFHE_REQUIRE_ALIGNED(out);
    const u64 count = len_in / f->n;
    if (count > 0x7fffffffull) return PFHE_ERR_BAD_LENGTH;
    DeviceGuard g(f->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return launch_groups(fft_inverse_kernel<W, true>, count, lds_bytes(f->log_n), s, (const double2 *)in, out, f->tw, f->log_n);
}

// host forms of the two transforms (in, out are host pointers)
template <class In, class Out, class DevFn>
int host_form(const pfhe_fft *f, const In *in, size_t in_bytes, Out *out, size_t out_bytes, size_t len_in, size_t len_out,
              DevFn dev) {
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    if ((!in && in_bytes) || (!out && out_bytes)) return PFHE_ERR_BAD_ARGUMENT;
    if (len_in % f->n != 0 || len_out != len_in) return PFHE_ERR_BAD_LENGTH;
    if (len_in == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(in, in_bytes), stage_out(out, out_bytes)};
    return staged_call(f->device, bufs, [&](void *const *d, hipStream_t s) { return dev((const In *)d[0], (Out *)d[1], s); });
}

// ---------------- plans ----------------

constexpr const char *kPlanBusy = "TFHE product plan in use by another thread (one plan per thread, like &mut TfheFftContext)";

// the shape on which the fused product and the whole-loop rotations run: it follows N and k alone
inline bool fused_shape(const Shape &sh) { return sh.k == 1 && sh.log_n <= kFusedMaxLogN; }

// the launches of the general product on `cur` ciphertexts behind the Hermitian parts in t.keyh: the digit transforms
// into t.spec, `mulacc` (the multiply-accumulate of the caller's form, which fills t.acc), the inverses into out
template <class W, class MulAcc>
int general_product(const pfhe_fft &f, const Shape &sh, const TfheProductScratch &t, const W *in, W *out, u64 cur, hipStream_t s,
                    MulAcc mulacc) {
    const u32 rows = sh.k + 1;
    PFHE_TRY(launch_groups(tfhe_digit_fwd_kernel<W>, cur * rows * sh.ell, lds_bytes(f.log_n), s, in, t.spec, f.tw, sh));
    PFHE_TRY(mulacc(cur * rows * (f.n / 2)));
    return launch_groups(fft_inverse_kernel<W, false>, cur * rows, lds_bytes(f.log_n), s, t.acc, out, f.tw, f.log_n);
}

}  // namespace

// What the CMUX handle (pfhe_cmux.hip) shares with the handles of this file: the create of a plan and the product's launches
// (declared in pfhe_tfhe_handles.hpp, instantiated at the end of this file)
namespace pfhe {

// P: a C handle (pfhe_tfhe{,32}_plan) or the core itself (the plan a rotation or a CMUX handle owns)
template <class W, class P>
int tfhe_plan_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t chunk,
                     P **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    Shape sh{};
    PFHE_TRY(tfhe_plan_check<W>(fft, glwe_dimension, log_basis, decompose_length, sh));
    auto p = std::make_unique<P>();
    p->shape = sh;
    p->fused = fused_shape(sh);
    p->chunk = chunk;
    DeviceGuard g(fft->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    p->fft = fft;
    PFHE_TRY(p->scratch.create(*fft, sh, 1, !p->fused, p->chunk));
    PFHE_TRY(p->guard.init(fft->device));
    *out = p.release();
    return PFHE_OK;
}

template <class W>
int tfhe_product_impl(TfhePlanCore<W> *p, const W *in, const double2 *key, W *out, u64 batch, hipStream_t s) {
    const pfhe_fft &f = *p->fft;
    const Shape &sh = p->shape;
    const TfheProductScratch &t = p->scratch;
    const u32 rows = sh.k + 1;
    const size_t glwe = (size_t)rows * f.n;
    if (!p->fused) PFHE_TRY(launch_flat(tfhe_key_herm_kernel, (u64)rows * sh.ell * rows * (f.n / 2), s, key, t.keyh, f.log_n));
    for (u64 done = 0; done < batch; done += p->chunk) {
        const u64 cur = std::min<u64>(p->chunk, batch - done);
        const W *x = in + done * glwe;
        W *o = out + done * glwe;
        if (p->fused) {
            PFHE_TRY(launch_groups(tfhe_fused_kernel<W>, cur, lds_bytes(f.log_n), s, x, key, o, f.tw, sh));
            continue;
        }
        PFHE_TRY(general_product<W>(f, sh, t, x, o, cur, s, [&](u64) {
            return tfhe_mulacc_launch(f, t.spec, t.keyh, t.acc, sh.k, sh.ell, sh.k + 1, cur, s);
        }));
    }
    return PFHE_OK;
}

}  // namespace pfhe

namespace {

// The host form refuses a null pointer before the lengths, and a wrong length without a message; the device form's
// pointer tests follow the empty batch.
template <class W>
int product(Form form, TfhePlanCore<W> *p, const W *in, size_t len_in, const double *key, size_t len_key, W *out,
            size_t len_out, hipStream_t s) {
    if (!p || !p->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(p->guard, kPlanBusy);
    if (form == Form::kHost && ((!in && len_in) || (!key && len_key) || (!out && len_out))) return PFHE_ERR_BAD_ARGUMENT;
    const pfhe_fft &f = *p->fft;
    const size_t rows = p->shape.k + 1, glwe = rows * f.n, key_len = rows * p->shape.ell * rows * f.n;
    if (len_in % glwe != 0 || len_out != len_in || len_key != key_len) {
        if (form == Form::kDevice)
            set_last_error("TFHE external product: input / output must be batch*(k+1)*N words and the key "
                           "(k+1)*ell*(k+1)*N complex values");
        return PFHE_ERR_BAD_LENGTH;
    }
    const u64 batch = len_in / glwe;
    if (batch == 0) return PFHE_OK;
    if (form == Form::kDevice) {
        if (!in || !key || !out) return PFHE_ERR_BAD_ARGUMENT;
        PFHE_REQUIRE_ALIGNED(in);
        PFHE_REQUIRE_ALIGNED(key);
        PFHE_REQUIRE_ALIGNED(out);
        // in place is safe: the fused form reads a ciphertext wholly before its workgroup writes it, the general form reads
        // a chunk's input in the digit launch and writes its output in the inverse launch
        if (in != out && overlaps(in, len_in * sizeof(W), out, len_out * sizeof(W))) {
            set_last_error("TFHE external product: input and output must be the same buffer or disjoint");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    const StageBuf bufs[] = {stage_in(in, len_in * sizeof(W)), stage_in(key, len_key * sizeof(double2)),
                             stage_out(out, len_out * sizeof(W))};
    return handle_call(p->guard, f.device, form, bufs, s, [&](void *const *d, hipStream_t st) {
        return tfhe_product_impl<W>(p, (const W *)d[0], (const double2 *)d[1], (W *)d[2], batch, st);
    });
}

// ---------------- blind rotation ----------------

constexpr const char *kBlindRotBusy = "TFHE blind-rotation handle in use by another thread (one handle per thread)";
constexpr const char *kBlindRotLengths = "TFHE blind rotation: acc must be batch*(k+1)*N words, bsk n_steps*(k+1)*ell*(k+1)*N "
                                         "complex values and exps batch*n_steps exponents";
constexpr size_t kDefaultGlueBytes = 256ull << 20;

enum class TorusGlue { kFirst, kFirstCopy, kStep, kLast, kMonomial };

template <class W, bool ADD_E, bool STORE_ACC, int ROT>
int launch_torus_glue(const W *acc, const W *e_in, W *acc_out, W *d_out, const u32 *exps, u32 exp_stride, u32 polys_per_exp,
                      u32 log_n, u64 total, hipStream_t s) {
    if (total == 0) return PFHE_OK;
    return launch_flat(tfhe_blindrot_glue_kernel<W, ADD_E, STORE_ACC, ROT>, total, s, acc, e_in, acc_out, d_out, exps, exp_stride,
                       polys_per_exp, log_n);
}

template <class W>
int torus_glue(const pfhe_fft &f, TorusGlue mode, const W *acc, const W *e_in, W *acc_out, W *d_out, const u32 *exps,
               u32 exp_stride, u32 polys_per_exp, u64 elements, hipStream_t s) {
    const u64 total = elements * polys_per_exp * f.n;
    switch (mode) {
        case TorusGlue::kFirst:
            return launch_torus_glue<W, false, false, kRotSub>(acc, nullptr, nullptr, d_out, exps, exp_stride, polys_per_exp,
                                                               f.log_n, total, s);
        case TorusGlue::kFirstCopy:
            return launch_torus_glue<W, false, true, kRotSub>(acc, nullptr, acc_out, d_out, exps, exp_stride, polys_per_exp,
                                                              f.log_n, total, s);
        case TorusGlue::kStep:
            return launch_torus_glue<W, true, true, kRotSub>(acc, e_in, acc_out, d_out, exps, exp_stride, polys_per_exp,
                                                             f.log_n, total, s);
        case TorusGlue::kLast:
            return launch_torus_glue<W, true, true, kRotNone>(acc, e_in, acc_out, nullptr, exps, exp_stride, polys_per_exp,
                                                              f.log_n, total, s);
        case TorusGlue::kMonomial:
            return launch_torus_glue<W, false, false, kRotOnly>(acc, nullptr, nullptr, d_out, exps, exp_stride, polys_per_exp,
                                                                f.log_n, total, s);
    }
    return PFHE_ERR_BAD_ARGUMENT;
}

// X^{exps[e]} * element e for `polys_per_exp` torus polynomials per element; out must not overlap a (the rotation reads
// a[(j - r) mod N] while other threads write out[j])
template <class W>
int torus_monomial_each(const pfhe_fft *f, const W *a, size_t len, const uint32_t *exps, size_t polys_per_exp, W *out,
                        hipStream_t s) {
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    const size_t unit = polys_per_exp * f->n;
    if (polys_per_exp == 0 || polys_per_exp > 0xffffffffull || len % unit != 0) {
        set_last_error("mul_monomial_each: len must be a whole number of elements of polys_per_exp * N words");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len == 0) return PFHE_OK;
    if (!a || !exps || !out) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(a);
    PFHE_REQUIRE_ALIGNED(out);
    if (overlaps(a, len * sizeof(W), out, len * sizeof(W))) {
        set_last_error("mul_monomial_each_to needs non-overlapping buffers");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    DeviceGuard g(f->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return torus_glue<W>(*f, TorusGlue::kMonomial, a, nullptr, nullptr, out, exps, 1, (u32)polys_per_exp, len / unit, s);
}

// tfhe_plan_create's checks in its order (the handle's plan IS a product plan), then the form: the whole-loop kernel on
// the product's fused shape unless PFHE_DISABLE_FUSED_TFHE_BLINDROT is set when the handle is created
template <class W, class H>
int tfhe_blindrot_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                         size_t chunk, H **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    auto h = std::make_unique<H>();
    TfhePlanCore<W> *plan = nullptr;
    PFHE_TRY(tfhe_plan_create<W>(fft, glwe_dimension, log_basis, decompose_length, chunk, &plan));
    h->plan.reset(plan);
    const TfhePlanCore<W> &p = *h->plan;
    h->fft = fft;
    h->glwe = (size_t)(p.shape.k + 1) * fft->n;
    h->key_len = (size_t)(p.shape.k + 1) * p.shape.ell * h->glwe;
    h->whole_loop = p.fused && std::getenv("PFHE_DISABLE_FUSED_TFHE_BLINDROT") == nullptr;
    h->chunk = p.chunk;
    DeviceGuard g(fft->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    if (!h->whole_loop) {
        // never above the plan's chunk, so a chunk of the rotation is one chunk of the product
        if (!chunk) h->chunk = std::min(p.chunk, std::max<size_t>(1, kDefaultGlueBytes / (3 * h->glwe * sizeof(W))));
        h->bufs.bind(fft->device);
        for (W **b : {&h->d, &h->e, &h->ping}) PFHE_TRY(h->bufs.add(*b, h->chunk * h->glwe));
    }
    PFHE_TRY(h->guard.init(fft->device));
    *out = h.release();
    return PFHE_OK;
}

template <class W>
int tfhe_blindrot_chunk(TfheBlindRotCore<W> *h, W *a0, const double2 *bsk, const uint32_t *ex, u64 n_steps, u64 cur,
                        hipStream_t s) {
    const pfhe_fft &f = *h->fft;
    if (h->whole_loop)
        return launch_groups(tfhe_blindrot_loop_kernel<W>, cur, lds_bytes(f.log_n) + h->glwe * sizeof(W), s, a0, bsk, ex,
                             (u32)n_steps, f.tw, h->plan->shape);
    // ping-pong between the caller's accumulator and the handle's: every step writes ACC' to the other one, so the gather
    // of a rotated word never sees a word already updated; an odd step count starts in the handle's buffer so that the
    // last step ends in the caller's
    const u32 rows = h->plan->shape.k + 1;
    W *src = a0;
    if (n_steps % 2) {
        PFHE_TRY(torus_glue<W>(f, TorusGlue::kFirstCopy, a0, nullptr, h->ping, h->d, ex, (u32)n_steps, rows, cur, s));
        src = h->ping;
    } else {
        PFHE_TRY(torus_glue<W>(f, TorusGlue::kFirst, a0, nullptr, nullptr, h->d, ex, (u32)n_steps, rows, cur, s));
    }
    for (u64 i = 0; i < n_steps; ++i) {
        PFHE_TRY(tfhe_product_impl<W>(h->plan.get(), h->d, bsk + i * h->key_len, h->e, cur, s));
        W *dst = src == a0 ? h->ping : a0;
        PFHE_TRY(i + 1 < n_steps
                     ? torus_glue<W>(f, TorusGlue::kStep, src, h->e, dst, h->d, ex + i + 1, (u32)n_steps, rows, cur, s)
                     : torus_glue<W>(f, TorusGlue::kLast, src, h->e, dst, nullptr, ex, (u32)n_steps, rows, cur, s));
        src = dst;
    }
    return PFHE_OK;
}

// The host form refuses a null pointer and an exponent of 2N or more before the lengths (the device form takes the
// exponents modulo 2N); the device form's pointer tests follow the empty batch and the cap on the steps.
template <class W>
int tfhe_blindrot(Form form, TfheBlindRotCore<W> *h, W *acc, size_t len_acc, const double *bsk, size_t len_bsk,
                  const uint32_t *exps, size_t len_exps, hipStream_t s) {
    if (!h || !h->plan) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kBlindRotBusy);
    if (form == Form::kHost) {
        if ((!acc && len_acc) || (!bsk && len_bsk) || (!exps && len_exps)) return PFHE_ERR_BAD_ARGUMENT;
        PFHE_TRY(require_exps_below_2n(exps, len_exps, h->fft->n, "TFHE blind rotation: every exponent must be below 2N"));
    }
    if (len_acc % h->glwe != 0 || len_bsk % h->key_len != 0 || len_exps != (len_acc / h->glwe) * (len_bsk / h->key_len)) {
        set_last_error(kBlindRotLengths);
        return PFHE_ERR_BAD_LENGTH;
    }
    const u64 batch = len_acc / h->glwe, n_steps = len_bsk / h->key_len;
    if (batch == 0 || n_steps == 0) return PFHE_OK;
    if (n_steps > 0xffffffffull) return PFHE_ERR_BAD_LENGTH;
    if (form == Form::kDevice) {
        if (!acc || !bsk || !exps) return PFHE_ERR_BAD_ARGUMENT;
        PFHE_REQUIRE_ALIGNED(acc);
        PFHE_REQUIRE_ALIGNED(bsk);
    }
    const StageBuf bufs[] = {stage_inout(acc, len_acc * sizeof(W)), stage_in(bsk, len_bsk * sizeof(double2)),
                             stage_in(exps, len_exps * sizeof(uint32_t))};
    return handle_call(h->guard, h->fft->device, form, bufs, s, [&](void *const *d, hipStream_t st) -> int {
        // chunk after chunk; every step of a chunk runs before the next chunk starts
        for (u64 done = 0; done < batch; done += h->chunk) {
            const u64 cur = std::min<u64>(h->chunk, batch - done);
            PFHE_TRY(tfhe_blindrot_chunk<W>(h, (W *)d[0] + done * h->glwe, (const double2 *)d[1],
                                            (const uint32_t *)d[2] + done * n_steps, n_steps, cur, st));
        }
        return PFHE_OK;
    });
}

// ---------------- multi-bit blind rotation ----------------

constexpr const char *kMbRotBusy = "TFHE multi-bit blind-rotation handle in use by another thread (one handle per thread)";
constexpr const char *kMbRotLengths = "TFHE multi-bit blind rotation: acc must be batch*(k+1)*N words, bsk groups*2^g keys of "
                                      "(k+1)*ell*(k+1)*N complex values and exps batch*groups*g exponents";
// the plan's checks in its order, then the grouping factor, all before the device (tfhe_mbrot_check); the whole-loop kernel
// on the product's fused shape unless PFHE_DISABLE_FUSED_TFHE_BLINDROT is set when the handle is created
template <class W, class H>
int tfhe_mbrot_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                      size_t grouping_factor, size_t chunk, H **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    Shape sh{};
    PFHE_TRY(tfhe_mbrot_check<W>(fft, glwe_dimension, log_basis, decompose_length, grouping_factor, sh));
    auto h = std::make_unique<H>();
    h->shape = sh;
    h->g = (u32)grouping_factor;
    h->glwe = (glwe_dimension + 1) * fft->n;
    h->key_len = (glwe_dimension + 1) * sh.ell * h->glwe;
    h->whole_loop = fused_shape(sh) && std::getenv("PFHE_DISABLE_FUSED_TFHE_BLINDROT") == nullptr;
    h->chunk = chunk;
    DeviceGuard g(fft->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    h->fft = fft;
    PFHE_TRY(h->scratch.create(*fft, sh, (size_t)1 << h->g, !h->whole_loop, h->chunk));
    PFHE_TRY(h->guard.init(fft->device));
    *out = h.release();
    return PFHE_OK;
}

// the launches of one rotation (arguments already checked)
template <class W>
int tfhe_mbrot_impl(TfheMultiBitCore<W> *h, W *acc, const double2 *bsk, const uint32_t *exps, u64 batch, u64 groups,
                    hipStream_t s) {
    const pfhe_fft &f = *h->fft;
    const Shape &sh = h->shape;
    const TfheProductScratch &t = h->scratch;
    const u32 rows = sh.k + 1, n_mask = (u32)(groups * h->g);
    // chunk after chunk; every group of a chunk runs before the next chunk starts.  Per group in the per-group form: the
    // Hermitian parts of its 2^g keys, then the product of ACC itself against the per-ciphertext key, back into ACC
    for (u64 done = 0; done < batch; done += h->chunk) {
        const u64 cur = std::min<u64>(h->chunk, batch - done);
        W *a = acc + done * h->glwe;
        const uint32_t *ex = exps + done * n_mask;
        if (h->whole_loop) {
            PFHE_TRY(launch_groups(tfhe_mb_blindrot_loop_kernel<W>, cur, lds_bytes(f.log_n) + h->glwe * sizeof(W), s, a, bsk, ex,
                                   (u32)groups, h->g, f.tw, sh));
            continue;
        }
        for (u64 g = 0; g < groups; ++g) {
            PFHE_TRY(launch_flat(tfhe_key_herm_kernel, ((u64)rows * sh.ell * rows * (f.n / 2)) << h->g, s,
                                 bsk + (g << h->g) * h->key_len, t.keyh, f.log_n));
            PFHE_TRY(general_product<W>(f, sh, t, a, a, cur, s, [&](u64 at) {
                return launch_flat(tfhe_mb_mulacc_kernel, at, s, t.spec, t.keyh, t.acc, ex + g * h->g, n_mask, h->g, f.tw,
                                   f.log_n, sh.k, sh.ell);
            }));
        }
    }
    return PFHE_OK;
}

template <class W>
bool mbrot_lengths_ok(const TfheMultiBitCore<W> *h, size_t len_acc, size_t len_bsk, size_t len_exps, u64 &batch, u64 &groups) {
    const size_t group_len = h->key_len << h->g;
    if (len_acc % h->glwe != 0 || len_bsk % group_len != 0) return false;
    batch = len_acc / h->glwe;
    groups = len_bsk / group_len;
    return len_exps == batch * groups * h->g;
}

// the refusals of the classic rotation, in its order
template <class W>
int tfhe_mbrot(Form form, TfheMultiBitCore<W> *h, W *acc, size_t len_acc, const double *bsk, size_t len_bsk,
               const uint32_t *exps, size_t len_exps, hipStream_t s) {
    if (!h || !h->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kMbRotBusy);
    if (form == Form::kHost) {
        if ((!acc && len_acc) || (!bsk && len_bsk) || (!exps && len_exps)) return PFHE_ERR_BAD_ARGUMENT;
        PFHE_TRY(require_exps_below_2n(exps, len_exps, h->fft->n, "TFHE multi-bit blind rotation: every exponent must be below 2N"));
    }
    u64 batch = 0, groups = 0;
    if (!mbrot_lengths_ok(h, len_acc, len_bsk, len_exps, batch, groups)) {
        set_last_error(kMbRotLengths);
        return PFHE_ERR_BAD_LENGTH;
    }
    if (batch == 0 || groups == 0) return PFHE_OK;
    if (groups * h->g > 0xffffffffull) return PFHE_ERR_BAD_LENGTH;
    if (form == Form::kDevice) {
        if (!acc || !bsk || !exps) return PFHE_ERR_BAD_ARGUMENT;
        PFHE_REQUIRE_ALIGNED(acc);
        PFHE_REQUIRE_ALIGNED(bsk);
    }
    const StageBuf bufs[] = {stage_inout(acc, len_acc * sizeof(W)), stage_in(bsk, len_bsk * sizeof(double2)),
                             stage_in(exps, len_exps * sizeof(uint32_t))};
    return handle_call(h->guard, h->fft->device, form, bufs, s, [&](void *const *d, hipStream_t st) {
        return tfhe_mbrot_impl<W>(h, (W *)d[0], (const double2 *)d[1], (const uint32_t *)d[2], batch, groups, st);
    });
}

// the combined key of one ciphertext and one group as a key in the reference's layout
int mb_combine_key_dev(const pfhe_fft *f, size_t glwe_dimension, size_t decompose_length, size_t grouping_factor,
                       const double *keys, size_t len_keys, const uint32_t *exps, size_t len_exps, double *out, size_t len_out,
                       hipStream_t s) {
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    if (glwe_dimension > kMaxGlweDimension) {
        set_last_error("glwe_dimension above 64 is not supported");
        return PFHE_ERR_UNSUPPORTED;
    }
    if (decompose_length == 0 || decompose_length > 64 || grouping_factor == 0 || grouping_factor > kMaxGrouping) {
        set_last_error("multi-bit key combination: decompose_length must be in 1..64 and grouping_factor in 1..4");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    const size_t rows = glwe_dimension + 1, key_len = rows * decompose_length * rows * f->n;
    if (len_keys != key_len << grouping_factor || len_exps != grouping_factor || len_out != key_len) {
        set_last_error("multi-bit key combination: keys must be 2^g keys of (k+1)*ell*(k+1)*N complex values, exps g exponents "
                       "and out one key");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (!keys || !exps || !out) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(keys);
    PFHE_REQUIRE_ALIGNED(out);
    if (overlaps(keys, len_keys * sizeof(double2), out, len_out * sizeof(double2))) {
        set_last_error("multi-bit key combination: the output must not overlap the keys");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    DeviceGuard g(f->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return launch_flat(tfhe_mb_combine_key_kernel, key_len / 2, s, (const double2 *)keys, exps, (double2 *)out,
                       (u32)grouping_factor, f->tw, f->log_n, (u64)key_len);
}

}  // namespace

// ---------------- the rotations as the bootstrap handle holds them ----------------

template <class W>
int TfheBlindRotCore<W>::rotate_dev(W *acc, size_t len_acc, const double *bsk, size_t len_bsk, const uint32_t *exps,
                                    size_t len_exps, hipStream_t s) {
    return tfhe_blindrot<W>(Form::kDevice, this, acc, len_acc, bsk, len_bsk, exps, len_exps, s);
}
template <class W>
int TfheMultiBitCore<W>::rotate_dev(W *acc, size_t len_acc, const double *bsk, size_t len_bsk, const uint32_t *exps,
                                    size_t len_exps, hipStream_t s) {
    return tfhe_mbrot<W>(Form::kDevice, this, acc, len_acc, bsk, len_bsk, exps, len_exps, s);
}

namespace pfhe {

template <class W>
int tfhe_rotation_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                         std::optional<size_t> grouping_factor, size_t chunk, TfheRotation<W> **out) {
    if (grouping_factor) {
        TfheMultiBitCore<W> *h = nullptr;
        const int rc = ::tfhe_mbrot_create<W>(fft, glwe_dimension, log_basis, decompose_length, *grouping_factor, chunk, &h);
        *out = h;
        return rc;
    }
    TfheBlindRotCore<W> *h = nullptr;
    const int rc = ::tfhe_blindrot_create<W>(fft, glwe_dimension, log_basis, decompose_length, chunk, &h);
    *out = h;
    return rc;
}
template int tfhe_rotation_create<u64>(const pfhe_fft *, size_t, uint32_t, size_t, std::optional<size_t>, size_t,
                                       TfheRotation<u64> **);
template int tfhe_rotation_create<u32>(const pfhe_fft *, size_t, uint32_t, size_t, std::optional<size_t>, size_t,
                                       TfheRotation<u32> **);

// ... and what pfhe_cmux.hip takes of the product: the create of the plan it owns and the launches
template int tfhe_plan_create<u64>(const pfhe_fft *, size_t, uint32_t, size_t, size_t, TfhePlanCore<u64> **);
template int tfhe_plan_create<u32>(const pfhe_fft *, size_t, uint32_t, size_t, size_t, TfhePlanCore<u32> **);
template int tfhe_product_impl<u64>(TfhePlanCore<u64> *, const u64 *, const double2 *, u64 *, u64, hipStream_t);
template int tfhe_product_impl<u32>(TfhePlanCore<u32> *, const u32 *, const double2 *, u32 *, u64, hipStream_t);

// ... and what the general form of pfhe_trace.hip takes: three launches of the general product as they are, on a key of
// k ell rows and on k digit rows per ciphertext
int tfhe_key_herm_launch(const pfhe_fft &f, const double2 *key, double2 *keyh, u64 polys, hipStream_t s) {
    return launch_flat(tfhe_key_herm_kernel, polys * (f.n / 2), s, key, keyh, f.log_n);
}
int tfhe_mulacc_launch(const pfhe_fft &f, const double2 *spec, const double2 *keyh, double2 *acc, u32 k, u32 ell, u32 in_rows,
                       u64 batch, hipStream_t s) {
    return launch_flat(tfhe_mulacc_kernel, batch * (k + 1) * (f.n / 2), s, spec, keyh, acc, f.log_n, k, ell, in_rows);
}
template <class W>
int tfhe_digit_fwd_launch(const pfhe_fft &f, const Shape &sh, const W *in, double2 *spec, u64 polys, hipStream_t s) {
    return launch_groups(tfhe_digit_fwd_kernel<W>, polys * sh.ell, lds_bytes(f.log_n), s, in, spec, f.tw, sh);
}
template <class W>
int tfhe_half_inverse_launch(const pfhe_fft &f, const double2 *acc, W *out, u64 polys, hipStream_t s) {
    return launch_groups(fft_inverse_kernel<W, false>, polys, lds_bytes(f.log_n), s, acc, out, f.tw, f.log_n);
}
template int tfhe_digit_fwd_launch<u64>(const pfhe_fft &, const Shape &, const u64 *, double2 *, u64, hipStream_t);
template int tfhe_digit_fwd_launch<u32>(const pfhe_fft &, const Shape &, const u32 *, double2 *, u64, hipStream_t);
template int tfhe_half_inverse_launch<u64>(const pfhe_fft &, const double2 *, u64 *, u64, hipStream_t);
template int tfhe_half_inverse_launch<u32>(const pfhe_fft &, const double2 *, u32 *, u64, hipStream_t);

}  // namespace pfhe

// The entry points of one word width.  P: pfhe_tfhe / pfhe_tfhe32; T: what the transforms' names call the width (torus /
// torus32); CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_FFT_FAMILY(P, T, CW, W)                                                                                  \
    PFHE_ENTRY(pfhe_fft_forward_##T##_dev, (const pfhe_fft *fft, const CW *input_dev, size_t len_input,               \
                double *output_dev, size_t len_output, void *stream),                                                 \
               forward_dev<W>(fft, (const W *)input_dev, len_input, output_dev, len_output, (hipStream_t)stream))     \
    PFHE_ENTRY(pfhe_fft_inverse_##T##_dev, (const pfhe_fft *fft, const double *input_dev, size_t len_input,           \
                CW *output_dev, size_t len_output, void *stream),                                                     \
               inverse_dev<W>(fft, input_dev, len_input, (W *)output_dev, len_output, (hipStream_t)stream))           \
    PFHE_ENTRY(pfhe_fft_forward_##T##_slice, (const pfhe_fft *fft, const CW *input, size_t len_input, double *output, \
                size_t len_output),                                                                                   \
               host_form(fft, input, len_input * sizeof(W), output, len_output * 16, len_input, len_output,           \
                         [&](const CW *a, double *b, hipStream_t s) {                                                 \
                             return forward_dev<W>(fft, (const W *)a, len_input, b, len_output, s);                   \
                         }))                                                                                          \
    PFHE_ENTRY(pfhe_fft_inverse_##T##_slice, (const pfhe_fft *fft, const double *input, size_t len_input, CW *output, \
                size_t len_output),                                                                                   \
               host_form(fft, input, len_input * 16, output, len_output * sizeof(W), len_input, len_output,           \
                         [&](const double *a, CW *b, hipStream_t s) {                                                 \
                             return inverse_dev<W>(fft, a, len_input, (W *)b, len_output, s);                         \
                         }))                                                                                          \
    PFHE_ENTRY(P##_plan_create, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                      \
                size_t decompose_length, size_t chunk, P##_plan **out),                                               \
               tfhe_plan_create<W>(fft, glwe_dimension, log_basis, decompose_length, chunk, out))                     \
    PFHE_HANDLE_TRIO(P##_plan, P##_plan, h->scratch.bytes())                                                          \
    PFHE_ENTRY(P##_external_product_to_dev, (P##_plan *plan, const CW *input_dev, size_t len_input,                   \
                const double *key_dev, size_t len_key, CW *output_dev, size_t len_output, void *stream),              \
               product<W>(Form::kDevice, plan, (const W *)input_dev, len_input, key_dev, len_key, (W *)output_dev,    \
                          len_output, (hipStream_t)stream))                                                           \
    PFHE_ENTRY(P##_external_product_to, (P##_plan *plan, const CW *input, size_t len_input, const double *key,        \
                size_t len_key, CW *output, size_t len_output),                                                       \
               product<W>(Form::kHost, plan, (const W *)input, len_input, key, len_key, (W *)output, len_output,      \
                          nullptr))                                                                                   \
    PFHE_ENTRY(P##_blindrot_create, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                  \
                size_t decompose_length, size_t chunk, P##_blindrot **out),                                           \
               tfhe_blindrot_create<W>(fft, glwe_dimension, log_basis, decompose_length, chunk, out))                 \
    PFHE_HANDLE_TRIO(P##_blindrot, P##_blindrot, h->scratch_bytes())                                                  \
    PFHE_ENTRY(P##_blindrot_rotate_dev, (P##_blindrot *h, CW *acc_dev, size_t len_acc, const double *bsk_dev,         \
                size_t len_bsk, const uint32_t *exps_dev, size_t len_exps, void *stream),                             \
               tfhe_blindrot<W>(Form::kDevice, h, (W *)acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps,        \
                                (hipStream_t)stream))                                                                 \
    PFHE_ENTRY(P##_blindrot_rotate, (P##_blindrot *h, CW *acc, size_t len_acc, const double *bsk, size_t len_bsk,     \
                const uint32_t *exps, size_t len_exps),                                                               \
               tfhe_blindrot<W>(Form::kHost, h, (W *)acc, len_acc, bsk, len_bsk, exps, len_exps, nullptr))            \
    PFHE_ENTRY(P##_mul_monomial_each_to_dev, (const pfhe_fft *fft, const CW *a_dev, size_t len,                       \
                const uint32_t *exps_dev, size_t polys_per_exp, CW *out_dev, void *stream),                           \
               torus_monomial_each<W>(fft, (const W *)a_dev, len, exps_dev, polys_per_exp, (W *)out_dev,              \
                                      (hipStream_t)stream))                                                           \
    PFHE_ENTRY(P##_mbrot_create, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                     \
                size_t decompose_length, size_t grouping_factor, size_t chunk, P##_mbrot **out),                      \
               tfhe_mbrot_create<W>(fft, glwe_dimension, log_basis, decompose_length, grouping_factor, chunk, out))   \
    PFHE_HANDLE_TRIO(P##_mbrot, P##_mbrot, h->scratch_bytes())                                                        \
    PFHE_ENTRY(P##_mbrot_rotate_dev, (P##_mbrot *h, CW *acc_dev, size_t len_acc, const double *bsk_dev,               \
                size_t len_bsk, const uint32_t *exps_dev, size_t len_exps, void *stream),                             \
               tfhe_mbrot<W>(Form::kDevice, h, (W *)acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps,           \
                             (hipStream_t)stream))                                                                    \
    PFHE_ENTRY(P##_mbrot_rotate, (P##_mbrot *h, CW *acc, size_t len_acc, const double *bsk, size_t len_bsk,           \
                const uint32_t *exps, size_t len_exps),                                                               \
               tfhe_mbrot<W>(Form::kHost, h, (W *)acc, len_acc, bsk, len_bsk, exps, len_exps, nullptr))

extern "C" {

PFHE_FFT_FAMILY(pfhe_tfhe, torus, uint64_t, u64)
PFHE_FFT_FAMILY(pfhe_tfhe32, torus32, uint32_t, u32)
#undef PFHE_FFT_FAMILY

/* ------------------------------ entry points without a word width ------------------------------ */

int pfhe_fft_create(uint32_t log_n, int device, pfhe_fft **out) {
    PFHE_GUARD_BEGIN
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (log_n == 0 || log_n > kMaxLogN) {
        set_last_error("FFT tables cover 1 <= log N <= 14 (the N/2-point transform of a polynomial lives in LDS)");
        return PFHE_ERR_UNSUPPORTED;
    }
    PFHE_TRY(capi_check_device(device));
    auto f = std::make_unique<pfhe_fft>();
    f->device = device;
    f->log_n = log_n;
    f->n = (size_t)1 << log_n;
    std::vector<double2> tw(f->n);
    const double nf = (double)f->n;
    for (size_t j = 0; j < f->n; ++j) {
        const double a = M_PI * (double)j / nf;  // Complex64::cis(PI * j as f64 / n_f64)
        tw[j] = make_double2(std::cos(a), std::sin(a));
    }
    DeviceGuard g(device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    f->bufs.bind(device);
    PFHE_TRY(f->bufs.add(f->tw, f->n));
    PFHE_HIP(hipMemcpy(f->tw, tw.data(), f->n * sizeof(double2), hipMemcpyHostToDevice));
    PFHE_TRY(set_lds_attributes<u64>(lds_bytes(log_n)));
    PFHE_TRY(set_lds_attributes<u32>(lds_bytes(log_n)));
    *out = f.release();
    return PFHE_OK;
    PFHE_GUARD_END
}
void pfhe_fft_destroy(pfhe_fft *fft) { delete fft; }
size_t pfhe_fft_poly_length(const pfhe_fft *fft) { return fft ? fft->n : 0; }
size_t pfhe_fft_fourier_length(const pfhe_fft *fft) { return fft ? fft->n : 0; }

int pfhe_tfhe_mb_combine_key_dev(const pfhe_fft *fft, size_t glwe_dimension, size_t decompose_length, size_t grouping_factor,
                                 const double *keys_dev, size_t len_keys, const uint32_t *exps_dev, size_t len_exps,
                                 double *out_dev, size_t len_out, void *stream) {
    PFHE_GUARD_BEGIN
    return mb_combine_key_dev(fft, glwe_dimension, decompose_length, grouping_factor, keys_dev, len_keys, exps_dev, len_exps,
                              out_dev, len_out, (hipStream_t)stream);
    PFHE_GUARD_END
}

}  // extern "C"
