// pfhe_trace.hip — moving a GLWE ciphertext: the Galois automorphism X -> X^t with its key switch, the plain GLWE key switch
// (t = 1), the homomorphic trace built from them, the keys they take and the embedding of an LWE ciphertext into a GLWE
// (include/pfhe.h: pfhe_tfhe{,32}_glwe_trace_*, _glwe_automorphism*, _glwe_trace*, _gksk_generate_dev, _lwe_embed*).
// No reference counterpart; DESIGN.md §21 states the rules.  All of it is the arithmetic of external_product_to
// (pfhe_fft.hip) with only the k mask rows decomposed; the product stays what it is.
//
//   sigma_t          p(X) -> p(X^t) mod X^N + 1 for odd t, exact on words: sigma_t(p)[i] = p[u] for u < N, -p[u - N]
//                    otherwise, u = i t^-1 mod 2N
//   rule 1, the automorphism   out = (0, .., 0, sigma_t(B)) - to_torus(sum_{j<k} sum_{l<ell} d_l(sigma_t(A_j)) key[j][l]),
//                    key the k ell mask rows of a Fourier GGSW: word for word sigma_t, the public product against the key
//                    padded with ell zero body rows, and a wrapping subtraction
//   rule 2, the trace   ACC_0 = in, ACC_s = ACC_{s-1} + automorphism(ACC_{s-1}, keys[s-1], 2^(log N - s + 1) + 1), s = 1..m
//   rule 3, the keys    row (j, l) of key x: B += sum_c A_c (*) key_out_c (the GLWE body call), B += g_l sigma_{t_x}(key_in_j)
//                    (tfhe_gksk_message_kernel), then the forward transform
//   rule 4, the embedding   A_j[0] = a[jN], A_j[N - i] = -a[jN + i], B = (b, 0, .., 0)
//   fused   (k = 1, N <= 2^11): tfhe_trace_loop_kernel, one launch per chunk for all steps, a workgroup per ciphertext,
//            ACC in LDS behind the digit spectrum, sigma_t as the row source of the product's own accumulate code;
//   general (every other shape): per step a gather launch, the product's digit, Hermitian-part and inverse launches on k
//            rows, a k-row multiply-accumulate and one subtract launch, over buffers the handle owns.  The slow form.
// Nothing is atomic and the summation order is the product's (mask rows, then levels; the padded product adds its zero
// rows, +-0, after them).  Launches and the two forms of both calls (handle_call) go through pfhe_tfhe_host.hpp.
#include <algorithm>
#include <cstdint>
#include <memory>

#include "pfhe_tfhe_handles.hpp"
#include "pfhe_trace_device.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// All steps of one ciphertext in one workgroup (k = 1, N <= 2^11): ACC (2N words) sits in LDS behind the digit spectrum
// from the first step to the last, as in tfhe_blindrot_loop_kernel.  Per step: sigma_t(A) and sigma_t(B) gathered from
// the LDS-resident ACC into registers, a barrier, B = [B +] sigma_t(B) at the thread's own slots (which frees those
// registers: held until the sink they would have to be picked by a run-time slot number, and the compiler then keeps them
// in scratch memory), the product's own accumulate code on the ONE mask row against the step's key of ell rows, its
// inverse code, and the sink: A = [A] - to_torus(E0), B -= to_torus(E1); the bracketed terms when the step accumulates.
// Every gather of a step precedes the step's first barrier and every store follows it; the sink's stores follow the
// barrier that ends fused_accumulate_rows, and fused_inverse_rows ends behind a barrier: no step reads a word the same
// step has already updated, and the input is read wholly before the output is written, so out may be exactly in.  (No
// __restrict__ on the two for that reason.)  The gather index i t^-1 has an odd stride: 64 consecutive i fall into 64
// different residues modulo 64, so the gather is expected to be free of LDS bank conflicts but for the split at the wrap.
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_trace_loop_kernel(const W *in, const double2 *__restrict__ keys, W *out,
                                                                   TraceSteps steps, const double2 *__restrict__ tw, Shape s) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_t[];
    const u32 n = 1u << s.log_n, m = n >> 1;
    W *a = reinterpret_cast<W *>(reinterpret_cast<char *>(lds_t) + lds_bytes(s.log_n));
    const W *g = in + (u64)blockIdx.x * 2 * n;
    W *o = out + (u64)blockIdx.x * 2 * n;
    for (u32 i = threadIdx.x; i < 2 * n; i += blockDim.x) a[i] = g[i];
    __syncthreads();
    const u64 key_len = (u64)2 * s.ell * n;
    const bool add = steps.accumulate != 0;
    for (u32 step = 0; step < steps.count; ++step) {
        const u32 t_inv = odd_inverse(steps.t[step], 2 * n - 1);
        double2 acc0[kFusedPer], acc1[kFusedPer];
        RegisterRow<W> mask;
        W body_lo[kFusedPer], body_hi[kFusedPer];
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) {
            const u32 i = threadIdx.x + u * kThreads;
            acc0[u] = acc1[u] = make_double2(0.0, 0.0);
            mask.a[u] = i < m ? sigma_word(a, i, t_inv, n) : (W)0;
            mask.b[u] = i < m ? sigma_word(a, i + m, t_inv, n) : (W)0;
            body_lo[u] = i < m ? sigma_word(a + n, i, t_inv, n) : (W)0;
            body_hi[u] = i < m ? sigma_word(a + n, i + m, t_inv, n) : (W)0;
        }
        __syncthreads();  // every gather of the step is done: B can take sigma_t(B) at the thread's own slots
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) {
            const u32 i = threadIdx.x + u * kThreads;
            if (i < m) {
                a[n + i] = (add ? a[n + i] : (W)0) + body_lo[u];
                a[n + i + m] = (add ? a[n + i + m] : (W)0) + body_hi[u];
            }
        }
        fused_accumulate_rows<W, 1>([&](u32) { return mask; }, ClassicKey{keys + step * key_len}, lds_t, tw, s, acc0, acc1);
        fused_inverse_rows(acc0, acc1, lds_t, tw, s, [&](u32 c, u32 i, double lo, double hi) {
            const bool keep = add || c;  // the body row already holds [B +] sigma_t(B)
            a[c * n + i] = (keep ? a[c * n + i] : (W)0) - to_torus<W>(lo);
            a[c * n + i + m] = (keep ? a[c * n + i + m] : (W)0) - to_torus<W>(hi);
        });
    }
    for (u32 i = threadIdx.x; i < 2 * n; i += blockDim.x) o[i] = a[i];
}

// ---------------- the general form ----------------

// One thread per word of `src` ((k+1) polynomials per ciphertext): sigma_t of the mask polynomials goes to d (k polynomials
// per ciphertext, what the digit launch walks), sigma_t(B) to body (one polynomial per ciphertext).
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_trace_gather_kernel(const W *__restrict__ src, W *__restrict__ d,
                                                                     W *__restrict__ body, u32 t_inv, u32 log_n, u32 k, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n, i = (u32)(t & (n - 1));
    const u64 poly = t >> log_n, e = poly / (k + 1);
    const u32 c = (u32)(poly - e * (k + 1));
    const W v = sigma_word(src + (poly << log_n), i, t_inv, n);
    if (c < k)
        d[((e * k + c) << log_n) + i] = v;
    else
        body[(e << log_n) + i] = v;
}

// One thread per word: dst = [src +] (0, .., 0, body) - e, the bracketed term when the step accumulates.  A thread reads
// and writes one index, so dst may be src.
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_trace_sub_kernel(const W *src, const W *__restrict__ body,
                                                                  const W *__restrict__ e_in, W *dst, u32 accumulate, u32 log_n,
                                                                  u32 k, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u64 poly = t >> log_n, e = poly / (k + 1);
    const u32 c = (u32)(poly - e * (k + 1)), i = (u32)(t & ((1u << log_n) - 1));
    W v = accumulate ? src[t] : (W)0;
    if (c == k) v += body[(e << log_n) + i];
    dst[t] = v - e_in[t];
}

// ---------------- the small kernels ----------------

// rule 3's message, one thread per word of the k ell bodies of ONE key: B of row (j, l) += sigma_t(key_in_j) << (drop + l
// log_basis)
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_gksk_message_kernel(W *__restrict__ key, const W *__restrict__ key_in, u32 t_inv,
                                                                     u32 log_n, u32 k, u32 ell, u32 log_basis, u32 drop,
                                                                     u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n, i = (u32)(t & (n - 1));
    const u64 row = t >> log_n;  // j ell + l
    const u32 j = (u32)(row / ell), l = (u32)(row % ell);
    key[((row * (k + 1) + k) << log_n) + i] += sigma_word(key_in + ((u64)j << log_n), i, t_inv, n) << (drop + l * log_basis);
}

// rule 4, one thread per output word
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_lwe_embed_kernel(const W *__restrict__ lwe, W *__restrict__ glwe, u32 log_n, u32 k,
                                                                  u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n, i = (u32)(t & (n - 1));
    const u64 poly = t >> log_n, e = poly / (k + 1);
    const u32 c = (u32)(poly - e * (k + 1));
    const W *x = lwe + e * (((u64)k << log_n) + 1);
    W v;
    if (c == k)
        v = i == 0 ? x[(u64)k << log_n] : (W)0;
    else
        v = i == 0 ? x[(u64)c << log_n] : (W)0 - x[((u64)c << log_n) + (n - i)];
    glwe[t] = v;
}

}  // namespace
}  // namespace pfhe

// ---------------- the handle ----------------

struct pfhe_tfhe_glwe_trace_handle : TfheTraceCore<u64> {};
struct pfhe_tfhe32_glwe_trace_handle : TfheTraceCore<u32> {};

namespace {

constexpr const char *kTraceBusy = "TFHE GLWE trace handle in use by another thread (one handle per thread)";
constexpr size_t kTraceDefaultBytes = 256ull << 20;

// the product plan's checks in their order, then the dimension, all before the device; then every allocation
template <class W, class H>
int trace_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t chunk, H **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    Shape sh{};
    PFHE_TRY(tfhe_plan_check<W>(fft, glwe_dimension, log_basis, decompose_length, sh));
    if (glwe_dimension == 0) {
        set_last_error("TFHE GLWE trace: glwe_dimension must be at least 1");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    auto h = std::make_unique<H>();
    h->shape = sh;
    h->fused = sh.k == 1 && sh.log_n <= kFusedMaxLogN;
    h->glwe = (glwe_dimension + 1) * fft->n;
    h->key_len = glwe_dimension * sh.ell * h->glwe;
    h->chunk = chunk;
    // the default chunk of the general form: the word buffers and the product's spectra and accumulators near 256 MiB
    const size_t per_ciphertext = 2 * h->glwe * sizeof(W) + (glwe_dimension + 1) * (sh.ell + 1) * (fft->n / 2) * sizeof(double2);
    if (!h->fused && !chunk) h->chunk = std::max<size_t>(1, kTraceDefaultBytes / per_ciphertext);
    DeviceGuard g(fft->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    h->fft = fft;
    PFHE_TRY(h->scratch.create(*fft, sh, 1, !h->fused, h->chunk));  // also caps the chunk at what a launch's grid holds
    if (!h->fused) {
        h->bufs.bind(fft->device);
        PFHE_TRY(h->bufs.add(h->d, h->chunk * sh.k * fft->n));
        PFHE_TRY(h->bufs.add(h->body, h->chunk * fft->n));
        PFHE_TRY(h->bufs.add(h->e, h->chunk * h->glwe));
    }
    PFHE_TRY(h->guard.init(fft->device));
    *out = h.release();
    return PFHE_OK;
}

}  // namespace

namespace pfhe {

// one step of the general form: a gather launch, the product's Hermitian-part, digit, multiply-accumulate and inverse
// launches on the k mask rows, and one subtract launch
template <class W>
int tfhe_trace_general_step(TfheTraceCore<W> *h, const W *gathered, const W *src, W *dst, const double2 *key, u32 t,
                            u32 accumulate, u64 cur, hipStream_t s) {
    const pfhe_fft &f = *h->fft;
    const Shape &sh = h->shape;
    const u32 k = sh.k;
    const u64 words = cur * h->glwe;
    const TfheProductScratch &p = h->scratch;
    PFHE_TRY(launch_flat(tfhe_trace_gather_kernel<W>, words, s, gathered, h->d, h->body, odd_inverse(t, 2 * (u32)f.n - 1), f.log_n, k));
    PFHE_TRY(tfhe_key_herm_launch(f, key, p.keyh, (u64)k * sh.ell * (k + 1), s));
    PFHE_TRY(tfhe_digit_fwd_launch<W>(f, sh, h->d, p.spec, cur * k, s));
    PFHE_TRY(tfhe_mulacc_launch(f, p.spec, p.keyh, p.acc, k, sh.ell, k, cur, s));
    PFHE_TRY(tfhe_half_inverse_launch<W>(f, p.acc, h->e, cur * (k + 1), s));
    return launch_flat(tfhe_trace_sub_kernel<W>, words, s, src, (const W *)h->body, (const W *)h->e, dst, accumulate, f.log_n, k);
}

// `steps` on `batch` ciphertexts, chunk after chunk, every step of a chunk queued before the next chunk starts.  keys: the
// steps' keys end to end.  Arguments are checked, the device is current.
template <class W>
int tfhe_trace_steps(TfheTraceCore<W> *h, const W *in, const double2 *keys, W *out, u64 batch, const TraceSteps &steps,
                     hipStream_t s) {
    const pfhe_fft &f = *h->fft;
    for (u64 done = 0; done < batch; done += h->chunk) {
        const u64 cur = std::min<u64>(h->chunk, batch - done);
        const W *x = in + done * h->glwe;
        W *o = out + done * h->glwe;
        if (h->fused) {
            PFHE_TRY(launch_groups(tfhe_trace_loop_kernel<W>, cur, lds_bytes(f.log_n) + 2 * f.n * sizeof(W), s, x, keys, o, steps, f.tw,
                                   h->shape));
            continue;
        }
        for (u32 st = 0; st < steps.count; ++st) {
            const W *src = st ? o : x;  // the first step reads the input, the rest the chunk's own output
            PFHE_TRY(tfhe_trace_general_step<W>(h, src, src, o, keys + (u64)st * h->key_len, steps.t[st], steps.accumulate, cur, s));
        }
    }
    return PFHE_OK;
}

template <class W>
int tfhe_trace_core_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t chunk,
                           TfheTraceCore<W> **out) {
    return trace_create<W>(fft, glwe_dimension, log_basis, decompose_length, chunk, out);
}

#define PFHE_TRACE_CORE(W)                                                                                                       \
    template int tfhe_trace_core_create<W>(const pfhe_fft *, size_t, uint32_t, size_t, size_t, TfheTraceCore<W> **);             \
    template int tfhe_trace_general_step<W>(TfheTraceCore<W> *, const W *, const W *, W *, const double2 *, u32, u32, u64,       \
                                            hipStream_t);                                                                        \
    template int tfhe_trace_steps<W>(TfheTraceCore<W> *, const W *, const double2 *, W *, u64, const TraceSteps &, hipStream_t);
PFHE_TRACE_CORE(u32)
PFHE_TRACE_CORE(u64)
#undef PFHE_TRACE_CORE

}  // namespace pfhe

namespace {

// What both calls of the handle share behind the lease and their own value check: steps.accumulate is the trace, whose out
// may be exactly in.  The host form refuses a null pointer before the lengths; the device form's pointer tests follow the
// empty batch.
template <class W>
int trace_call(Form form, TfheTraceCore<W> *h, const W *in, size_t len_in, const double *keys, size_t len_keys, W *out,
               size_t len_out, const TraceSteps &steps, const char *lengths, hipStream_t s) {
    if (form == Form::kHost && ((!in && len_in) || (!keys && len_keys) || (!out && len_out))) return PFHE_ERR_BAD_ARGUMENT;
    if (len_in % h->glwe != 0 || len_out != len_in || len_keys != steps.count * h->key_len) {
        set_last_error(lengths);
        return PFHE_ERR_BAD_LENGTH;
    }
    const u64 batch = len_in / h->glwe;
    if (batch == 0) return PFHE_OK;
    if (form == Form::kDevice) {
        if (!in || !keys || !out) return PFHE_ERR_BAD_ARGUMENT;
        PFHE_REQUIRE_ALIGNED(in);
        PFHE_REQUIRE_ALIGNED(keys);
        PFHE_REQUIRE_ALIGNED(out);
        const size_t bytes = len_out * sizeof(W);
        // the trace reads a ciphertext (a chunk, in the general form) wholly before it writes it; rule 1 alone is a gather
        const bool alias_ok = steps.accumulate && in == out;
        if ((!alias_ok && overlaps(in, bytes, out, bytes)) || overlaps(keys, len_keys * sizeof(double2), out, bytes)) {
            set_last_error(steps.accumulate ? "TFHE GLWE trace: out must be exactly in or disjoint from it, and disjoint from the keys"
                                            : "TFHE GLWE automorphism: out must overlap neither in (the operation is a gather) nor the key");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    const StageBuf bufs[] = {stage_in(in, len_in * sizeof(W)), stage_in(keys, len_keys * sizeof(double2)),
                             stage_out(out, len_out * sizeof(W))};
    return handle_call(h->guard, h->fft->device, form, bufs, s, [&](void *const *p, hipStream_t st) {
        return tfhe_trace_steps<W>(h, (const W *)p[0], (const double2 *)p[1], (W *)p[2], batch, steps, st);
    });
}

template <class W>
int automorphism(Form form, TfheTraceCore<W> *h, const W *in, size_t len_in, const double *key, size_t len_key, uint32_t t, W *out,
                 size_t len_out, hipStream_t s) {
    if (!h || !h->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kTraceBusy);
    if ((t & 1) == 0 || t >= 2 * h->fft->n) {
        set_last_error("TFHE GLWE automorphism: t must be odd and in 1..2N-1");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    TraceSteps steps{1, 0, {t}};
    return trace_call<W>(form, h, in, len_in, key, len_key, out, len_out, steps,
                         "TFHE GLWE automorphism: in and out must be batch*(k+1)*N words and the key k*ell*(k+1)*N complex values", s);
}

template <class W>
int trace(Form form, TfheTraceCore<W> *h, const W *in, size_t len_in, const double *keys, size_t len_keys, size_t m, W *out,
          size_t len_out, hipStream_t s) {
    if (!h || !h->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kTraceBusy);
    const u32 log_n = h->fft->log_n;
    if (m == 0 || m > log_n) {
        set_last_error("TFHE GLWE trace: steps must be in 1..log N");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    TraceSteps steps{(u32)m, 1, {}};
    for (u32 st = 1; st <= m; ++st) steps.t[st - 1] = (1u << (log_n - st + 1)) + 1;
    return trace_call<W>(form, h, in, len_in, keys, len_keys, out, len_out, steps,
                         "TFHE GLWE trace: in and out must be batch*(k+1)*N words and keys steps*k*ell*(k+1)*N complex values", s);
}

// ---------------- the stateless calls ----------------

inline int forward_torus(const pfhe_fft *f, const u64 *in, size_t len, double *out, hipStream_t s) {
    return pfhe_fft_forward_torus_dev(f, (const uint64_t *)in, len, out, len, s);
}
inline int forward_torus(const pfhe_fft *f, const u32 *in, size_t len, double *out, hipStream_t s) {
    return pfhe_fft_forward_torus32_dev(f, in, len, out, len, s);
}

// the product plan's checks, the dimension, the exponents (host values), the lengths; then the stateless tail
template <class W>
int gksk_generate_dev(const pfhe_fft *f, size_t k, uint32_t log_basis, size_t decompose_length, const W *key_in, size_t len_key_in,
                      const W *key_out, size_t len_key_out, const uint32_t *exponents, size_t count, W *gksk, size_t len,
                      double *out, size_t len_out, hipStream_t s) {
    Shape sh{};
    PFHE_TRY(tfhe_plan_check<W>(f, k, log_basis, decompose_length, sh));
    if (k == 0) {
        set_last_error("GLWE key-switch key: glwe_dimension must be at least 1");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (!exponents && count) return PFHE_ERR_BAD_ARGUMENT;
    for (size_t x = 0; x < count; ++x) {
        if ((exponents[x] & 1) == 0 || exponents[x] >= 2 * f->n) {
            set_last_error("GLWE key-switch key: every exponent must be odd and in 1..2N-1");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    const size_t rows = k * sh.ell, one = rows * (k + 1) * f->n;
    if (len_key_in != k * f->n || len_key_out != k * f->n || len != count * one || len_out != len) {
        set_last_error("GLWE key-switch key: both keys must be k*N words, gksk_torus count*k*ell*(k+1)*N words and gksk_out as many "
                       "complex values");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(key_in, len_key_in * sizeof(W)), stage_in(key_out, len_key_out * sizeof(W)),
                             stage_inout(gksk, len * sizeof(W)), stage_out(out, len_out * 2 * sizeof(double))};
    PFHE_TRY(refuse_null(bufs));  // ahead of the tail's own: the alignment is judged between the null and the overlap test
    PFHE_REQUIRE_ALIGNED(gksk);
    PFHE_REQUIRE_ALIGNED(out);
    return stateless_call(
        f->device, Form::kDevice, bufs, "GLWE key-switch key: the outputs must overlap neither each other nor a key", s,
        [&](void *const *d, hipStream_t st) {
            PFHE_TRY(glwe_body_add(f, k, (W *)d[2], len, (const W *)d[1], len_key_out, st));
            for (size_t x = 0; x < count; ++x)
                PFHE_TRY(launch_flat(tfhe_gksk_message_kernel<W>, (u64)rows * f->n, st, (W *)d[2] + x * one, (const W *)d[0],
                                     odd_inverse(exponents[x], 2 * (u32)f->n - 1), f->log_n, (u32)k, sh.ell, log_basis, sh.drop_bits));
            return forward_torus(f, (const W *)d[2], len, (double *)d[3], st);
        },
        [&] { return count * rows > 0x7fffffffull || len / f->n > 0x7fffffffull ? PFHE_ERR_BAD_LENGTH : PFHE_OK; });
}

template <class W>
int lwe_embed(Form form, const pfhe_fft *f, size_t k, const W *lwe, size_t len_lwe, W *glwe, size_t len_glwe, hipStream_t s) {
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_TRY(require_glwe_dimension(k, "LWE embedding: glwe_dimension must be in 1..64"));
    const size_t in_words = k * f->n + 1, out_words = (k + 1) * f->n;
    if (len_lwe % in_words != 0 || len_glwe != len_lwe / in_words * out_words) {
        set_last_error("LWE embedding: lwe must be batch*(k*N+1) words and glwe_out batch*(k+1)*N");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_lwe == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(lwe, len_lwe * sizeof(W)), stage_out(glwe, len_glwe * sizeof(W))};
    return stateless_call(f->device, form, bufs, "LWE embedding: the output must not overlap the input", s,
                          [&](void *const *d, hipStream_t st) {
                              return launch_flat(tfhe_lwe_embed_kernel<W>, (u64)len_glwe, st, (const W *)d[0], (W *)d[1], f->log_n,
                                                 (u32)k);
                          });
}

template <class H>
size_t trace_scratch(const H *h) {
    return h && h->fft ? h->bufs.bytes() + h->scratch.bytes() : 0;
}

}  // namespace

// The entry points of one word width.  P: pfhe_tfhe / pfhe_tfhe32; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_TRACE_FAMILY(P, CW, W)                                                                                      \
    PFHE_ENTRY(P##_glwe_trace_create, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                   \
                size_t decompose_length, size_t chunk, P##_glwe_trace_handle **out),                                     \
               trace_create<W>(fft, glwe_dimension, log_basis, decompose_length, chunk, out))                            \
    PFHE_HANDLE_TRIO(P##_glwe_trace, P##_glwe_trace_handle, trace_scratch(h))                                            \
    PFHE_ENTRY(P##_glwe_automorphism_dev, (P##_glwe_trace_handle *h, const CW *in_dev, size_t len_in,                    \
                const double *key_dev, size_t len_key, uint32_t t, CW *out_dev, size_t len_out, void *stream),           \
               automorphism<W>(Form::kDevice, h, (const W *)in_dev, len_in, key_dev, len_key, t, (W *)out_dev, len_out,  \
                               (hipStream_t)stream))                                                                     \
    PFHE_ENTRY(P##_glwe_automorphism, (P##_glwe_trace_handle *h, const CW *in, size_t len_in, const double *key,         \
                size_t len_key, uint32_t t, CW *out, size_t len_out),                                                    \
               automorphism<W>(Form::kHost, h, (const W *)in, len_in, key, len_key, t, (W *)out, len_out, nullptr))      \
    PFHE_ENTRY(P##_glwe_trace_dev, (P##_glwe_trace_handle *h, const CW *in_dev, size_t len_in, const double *keys_dev,   \
                size_t len_keys, size_t steps, CW *out_dev, size_t len_out, void *stream),                               \
               trace<W>(Form::kDevice, h, (const W *)in_dev, len_in, keys_dev, len_keys, steps, (W *)out_dev, len_out,   \
                        (hipStream_t)stream))                                                                            \
    PFHE_ENTRY(P##_glwe_trace, (P##_glwe_trace_handle *h, const CW *in, size_t len_in, const double *keys,               \
                size_t len_keys, size_t steps, CW *out, size_t len_out),                                                 \
               trace<W>(Form::kHost, h, (const W *)in, len_in, keys, len_keys, steps, (W *)out, len_out, nullptr))       \
    PFHE_ENTRY(P##_gksk_generate_dev, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                   \
                size_t decompose_length, const CW *key_in_dev, size_t len_key_in, const CW *key_out_dev,                 \
                size_t len_key_out, const uint32_t *exponents, size_t count, CW *gksk_torus_dev, size_t len_gksk,        \
                double *gksk_out_dev, size_t len_out, void *stream),                                                     \
               gksk_generate_dev<W>(fft, glwe_dimension, log_basis, decompose_length, (const W *)key_in_dev, len_key_in, \
                                    (const W *)key_out_dev, len_key_out, exponents, count, (W *)gksk_torus_dev,          \
                                    len_gksk, gksk_out_dev, len_out, (hipStream_t)stream))                               \
    PFHE_ENTRY(P##_lwe_embed_dev, (const pfhe_fft *fft, size_t glwe_dimension, const CW *lwe_dev, size_t len_lwe,        \
                CW *glwe_out_dev, size_t len_out, void *stream),                                                         \
               lwe_embed<W>(Form::kDevice, fft, glwe_dimension, (const W *)lwe_dev, len_lwe, (W *)glwe_out_dev, len_out, \
                            (hipStream_t)stream))                                                                        \
    PFHE_ENTRY(P##_lwe_embed, (const pfhe_fft *fft, size_t glwe_dimension, const CW *lwe, size_t len_lwe,                \
                CW *glwe_out, size_t len_out),                                                                           \
               lwe_embed<W>(Form::kHost, fft, glwe_dimension, (const W *)lwe, len_lwe, (W *)glwe_out, len_out, nullptr))

extern "C" {

PFHE_TRACE_FAMILY(pfhe_tfhe, uint64_t, u64)
PFHE_TRACE_FAMILY(pfhe_tfhe32, uint32_t, u32)
#undef PFHE_TRACE_FAMILY

}  // extern "C"
