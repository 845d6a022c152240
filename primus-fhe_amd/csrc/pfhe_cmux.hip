// pfhe_cmux.hip — the batched CMUX with a Fourier GGSW selector per group of ciphertexts, and the tree of CMUXes that
// selects one of 2^d GLWE ciphertexts by d encrypted bits (include/pfhe.h: pfhe_tfhe{,32}_cmux_tree_*, _cmux, _cmux_dev).
// No reference counterpart; DESIGN.md §20 states the rules.  Both are built on the arithmetic of external_product_to
// (pfhe_fft.hip), which stays what it is.
//
//   rule 1, the CMUX     out[i] = d0[i] + external_product_to(d1[i] - d0[i], keys[i / per_key]) modulo 2^BITS
//   rule 2, the tree     level j = 0..d-1 of input e: node_{j+1}[e][i] = CMUX(node_j[e][2i], node_j[e][2i+1]; selectors[e d + j]),
//                        node_0[e] the table (one for the batch, or one per input), out[e] = node_d[e][0]: d calls of
//                        rule 1 with per_key = 2^(d-1-j) and a key stride of d.
//   fused   (k = 1, N <= 2^11): tfhe_cmux_kernel, one launch per level and chunk, a workgroup per node: the difference in
//            registers, the product's own accumulate and inverse code against the node's key, d0 added in the sink;
//   general (every other shape): one difference launch, the product's own launch sequence (tfhe_product_impl) once per key
//            group on a plan the handle owns, one add launch, all under the handle's own stream order.  batch * d product
//            sequences per tree: the slow form.
// Nothing is atomic and the summation order is the product's: the words depend neither on the batch, nor on the chunk,
// nor on how per_key tiles the launches.  Launches and the two forms of both calls (handle_call) go through
// pfhe_tfhe_host.hpp.  The look-up handle (pfhe_lut.hip) owns a TfheCmuxTreeCore of its own and runs rule 1 on it through
// tfhe_cmux_core_create / tfhe_cmux_launch at the end of this file.
#include <algorithm>
#include <cstdint>
#include <memory>

#include "pfhe_tfhe_handles.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// Where a launch finds its nodes.  Node b of the launch (blockIdx.x) reads d0 / d1 at index (b mod period) * stride words
// (period 0: b itself; a period is the shared table of the tree's first level) and writes out at b * (k+1) N.  Its key is
// keys + ((first_node + b) / per_key) * key_stride: first_node is the global index of the launch's first node, so a chunk
// boundary inside a key group still picks the group's key.
struct CmuxNodes {
    u64 stride, first_node, per_key, key_stride;
    u32 period;
    __device__ __forceinline__ u64 source(u64 b) const { return (period ? b % period : b) * stride; }
    __device__ __forceinline__ u64 key(u64 b) const { return ((first_node + b) / per_key) * key_stride; }
};

// One workgroup per CMUX node (k = 1, N <= 2^11); the body is pfhe_fft_device.hpp's fused_accumulate_rows /
// fused_inverse_rows, so the product inside is the fused product's arithmetic, operation for operation.  Every read of
// d0 / d1 by the row source precedes a barrier of fused_accumulate_rows, every store of the sink follows the barrier that
// ends it, and the sink reads d0 at the index it then writes, in the same thread: out may be exactly d0 or exactly d1.
// (No __restrict__ on the three for that reason.)
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_cmux_kernel(const W *d0, const W *d1, const double2 *__restrict__ keys,
                                                             W *out, const double2 *__restrict__ tw, Shape s, CmuxNodes nodes) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_c[];
    const u32 n = 1u << s.log_n, m = n >> 1;
    const u64 src = nodes.source(blockIdx.x);
    const W *x0 = d0 + src, *x1 = d1 + src;
    W *o = out + (u64)blockIdx.x * 2 * n;
    double2 acc0[kFusedPer], acc1[kFusedPer];
#pragma unroll
    for (int u = 0; u < kFusedPer; ++u) acc0[u] = acc1[u] = make_double2(0.0, 0.0);
    fused_accumulate_rows<W>([&](u32 row) {
        RegisterRow<W> d;  // D = d1 - d0, formed once and held in registers for all its levels
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) {
            const u32 i = threadIdx.x + u * kThreads;
            d.a[u] = i < m ? (W)(x1[row * n + i] - x0[row * n + i]) : (W)0;
            d.b[u] = i < m ? (W)(x1[row * n + i + m] - x0[row * n + i + m]) : (W)0;
        }
        return d;
    }, ClassicKey{keys + nodes.key(blockIdx.x)}, lds_c, tw, s, acc0, acc1);
    fused_inverse_rows(acc0, acc1, lds_c, tw, s, [&](u32 c, u32 i, double lo, double hi) {
        o[c * n + i] = x0[c * n + i] + to_torus<W>(lo);
        o[c * n + i + m] = x0[c * n + i + m] + to_torus<W>(hi);
    });
}

// The element-wise ends of the general form, one thread per word of `glwe` words per node: ADD false, out = d1 - d0 (the
// handle's D buffer); ADD true, out = d0 + e (d1 is then the handle's E buffer, read at the node's own index).  A thread
// reads and writes one index, so the add may store over d0 or d1.
template <class W, bool ADD>
__global__ __launch_bounds__(kThreads) void tfhe_cmux_glue_kernel(const W *d0, const W *d1, W *out, u64 glwe, CmuxNodes nodes,
                                                                  u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u64 b = t / glwe, j = t - b * glwe;
    const W a = d0[nodes.source(b) + j];
    out[t] = ADD ? (W)(a + d1[t]) : (W)(d1[nodes.source(b) + j] - a);
}

}  // namespace
}  // namespace pfhe

// ---------------- the handle ----------------

// TfheCmuxTreeCore (pfhe_tfhe_handles.hpp) is what a handle owns; the look-up handle (pfhe_lut.hip) owns one too.
struct pfhe_tfhe_cmux_tree_handle : TfheCmuxTreeCore<u64> {};
struct pfhe_tfhe32_cmux_tree_handle : TfheCmuxTreeCore<u32> {};

namespace {

constexpr const char *kCmuxBusy = "TFHE CMUX-tree handle in use by another thread (one handle per thread)";
constexpr const char *kCmuxLengths = "TFHE CMUX: d0, d1 and out must be count*(k+1)*N words, count a multiple of per_key, and "
                                     "keys (count/per_key)*(k+1)*ell*(k+1)*N complex values";
constexpr const char *kTreeLengths = "TFHE CMUX tree: out must be batch*(k+1)*N words, selectors batch*depth keys of "
                                     "(k+1)*ell*(k+1)*N complex values and table 2^depth or batch*2^depth ciphertexts";
constexpr size_t kCmuxDefaultBytes = 256ull << 20;
constexpr size_t kMaxDepth = 16;

// the product plan's checks in their order, then the depth, all before the device; then every allocation
template <class W>
int cmux_core_init(TfheCmuxTreeCore<W> *h, const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,
                   size_t decompose_length, size_t depth, size_t chunk) {
    Shape sh{};
    PFHE_TRY(tfhe_plan_check<W>(fft, glwe_dimension, log_basis, decompose_length, sh));
    if (depth == 0 || depth > kMaxDepth) {
        set_last_error("TFHE CMUX tree: depth must be in 1..16");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    h->shape = sh;
    h->depth = (u32)depth;
    h->fused = sh.k == 1 && sh.log_n <= kFusedMaxLogN;
    h->glwe = (glwe_dimension + 1) * fft->n;
    h->key_len = (glwe_dimension + 1) * sh.ell * h->glwe;
    // ciphertexts per input: the two node buffers (one ciphertext stands for them at depth 1), and D and E in the general form
    const size_t half = (size_t)1 << (depth - 1), nodes = depth > 1 ? half + half / 2 : 0;
    const size_t per_input = std::max<size_t>(1, nodes) + (h->fused ? 0 : 2 * half);
    h->chunk = chunk ? chunk : std::max<size_t>(1, kCmuxDefaultBytes / (per_input * h->glwe * sizeof(W)));
    if (h->chunk > (0x7fffffffull >> (depth - 1))) {
        if (chunk) return PFHE_ERR_BAD_LENGTH;
        h->chunk = 0x7fffffffull >> (depth - 1);  // a launch's grid holds chunk * 2^(depth-1) nodes
    }
    DeviceGuard g(fft->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    h->fft = fft;
    const size_t level = h->chunk * half * h->glwe;  // words of the widest level's nodes
    h->bufs.bind(fft->device);
    PFHE_TRY(h->bufs.add(h->node[0], depth > 1 ? level : 0));
    PFHE_TRY(h->bufs.add(h->node[1], depth > 2 ? level / 2 : 0));
    PFHE_TRY(h->bufs.add(h->d, h->fused ? 0 : level));
    PFHE_TRY(h->bufs.add(h->e, h->fused ? 0 : level));
    if (!h->fused) {
        TfhePlanCore<W> *plan = nullptr;
        PFHE_TRY(tfhe_plan_create<W>(fft, glwe_dimension, log_basis, decompose_length, 0, &plan));
        h->plan.reset(plan);
    }
    return h->guard.init(fft->device);
}

template <class W, class H>
int cmux_tree_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t depth,
                     size_t chunk, H **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    auto h = std::make_unique<H>();
    PFHE_TRY(cmux_core_init<W>(h.get(), fft, glwe_dimension, log_basis, decompose_length, depth, chunk));
    *out = h.release();
    return PFHE_OK;
}

// Rule 1 on `count` nodes whose sources `at` describes (stride, period, per_key, key_stride; first_node is set here), at most
// launch_nodes() of them per launch; out is count ciphertexts.  Arguments are checked, the device is current.
template <class W>
int cmux_nodes(TfheCmuxTreeCore<W> *h, const W *d0, const W *d1, const double2 *keys, W *out, u64 count, CmuxNodes at,
               hipStream_t s) {
    const pfhe_fft &f = *h->fft;
    for (u64 done = 0; done < count; done += h->launch_nodes()) {
        const u64 cur = std::min<u64>(h->launch_nodes(), count - done);
        // a period divides every launch's first node (the tree's chunks are whole inputs), so a launch starts at source 0
        const u64 off = at.period ? 0 : done * at.stride;
        W *o = out + done * h->glwe;
        at.first_node = done;
        if (h->fused) {
            PFHE_TRY(launch_groups(tfhe_cmux_kernel<W>, cur, lds_bytes(f.log_n), s, d0 + off, d1 + off, keys, o, f.tw, h->shape, at));
            continue;
        }
        PFHE_TRY(launch_flat(tfhe_cmux_glue_kernel<W, false>, cur * h->glwe, s, d0 + off, d1 + off, h->d, (u64)h->glwe, at));
        for (u64 b = 0; b < cur;) {  // the product's own launches, once per key group that the launch meets
            const u64 group = (done + b) / at.per_key;
            const u64 run = std::min<u64>(cur - b, (group + 1) * at.per_key - (done + b));
            PFHE_TRY(tfhe_product_impl<W>(h->plan.get(), h->d + b * h->glwe, keys + group * at.key_stride, h->e + b * h->glwe, run, s));
            b += run;
        }
        PFHE_TRY(launch_flat(tfhe_cmux_glue_kernel<W, true>, cur * h->glwe, s, d0 + off, (const W *)h->e, o, (u64)h->glwe, at));
    }
    return PFHE_OK;
}

// The host form refuses a null pointer before the lengths; the device form's pointer tests follow the empty batch.
template <class W>
int cmux(Form form, TfheCmuxTreeCore<W> *h, const W *d0, size_t len_d0, const W *d1, size_t len_d1, const double *keys,
         size_t len_keys, size_t per_key, W *out, size_t len_out, hipStream_t s) {
    if (!h || !h->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kCmuxBusy);
    if (form == Form::kHost && ((!d0 && len_d0) || (!d1 && len_d1) || (!keys && len_keys) || (!out && len_out)))
        return PFHE_ERR_BAD_ARGUMENT;
    const u64 count = len_d0 / h->glwe;
    if (per_key == 0 || len_d0 % h->glwe != 0 || len_d1 != len_d0 || len_out != len_d0 || count % per_key != 0 ||
        len_keys != count / per_key * h->key_len) {
        set_last_error(kCmuxLengths);
        return PFHE_ERR_BAD_LENGTH;
    }
    if (count == 0) return PFHE_OK;
    if (form == Form::kDevice) {
        if (!d0 || !d1 || !keys || !out) return PFHE_ERR_BAD_ARGUMENT;
        PFHE_REQUIRE_ALIGNED(d0);
        PFHE_REQUIRE_ALIGNED(d1);
        PFHE_REQUIRE_ALIGNED(keys);
        PFHE_REQUIRE_ALIGNED(out);
        // in place is safe (tfhe_cmux_kernel; the general form reads both inputs in the difference launch and adds index by
        // index)
        const size_t bytes = len_out * sizeof(W);
        if ((out != d0 && overlaps(d0, bytes, out, bytes)) || (out != d1 && overlaps(d1, bytes, out, bytes)) ||
            overlaps(keys, len_keys * sizeof(double2), out, bytes)) {
            set_last_error("TFHE CMUX: out must be exactly d0, exactly d1, or disjoint from both, and disjoint from the keys");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    const StageBuf bufs[] = {stage_in(d0, len_d0 * sizeof(W)), stage_in(d1, len_d1 * sizeof(W)),
                             stage_in(keys, len_keys * sizeof(double2)), stage_out(out, len_out * sizeof(W))};
    return handle_call(h->guard, h->fft->device, form, bufs, s, [&](void *const *p, hipStream_t st) {
        return cmux_nodes<W>(h, (const W *)p[0], (const W *)p[1], (const double2 *)p[2], (W *)p[3], count,
                             CmuxNodes{h->glwe, 0, per_key, h->key_len, 0}, st);
    });
}

// batch from the output; the table is shared when it holds 2^d ciphertexts (at batch 1 the two readings coincide)
template <class W>
bool tree_lengths_ok(const TfheCmuxTreeCore<W> *h, size_t len_table, size_t len_selectors, size_t len_out, u64 &batch,
                     bool &shared) {
    if (len_out % h->glwe != 0) return false;
    batch = len_out / h->glwe;
    const size_t leaves = h->glwe << h->depth;
    shared = len_table == leaves;
    return len_selectors == batch * h->depth * h->key_len && (shared || len_table == batch * leaves);
}

// the refusals of the CMUX, in its order
template <class W>
int cmux_tree(Form form, TfheCmuxTreeCore<W> *h, const W *table, size_t len_table, const double *selectors, size_t len_selectors,
              W *out, size_t len_out, hipStream_t s) {
    if (!h || !h->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kCmuxBusy);
    if (form == Form::kHost && ((!table && len_table) || (!selectors && len_selectors) || (!out && len_out)))
        return PFHE_ERR_BAD_ARGUMENT;
    u64 batch = 0;
    bool shared = false;
    if (!tree_lengths_ok(h, len_table, len_selectors, len_out, batch, shared)) {
        set_last_error(kTreeLengths);
        return PFHE_ERR_BAD_LENGTH;
    }
    if (batch == 0) return PFHE_OK;
    if (form == Form::kDevice) {
        if (!table || !selectors || !out) return PFHE_ERR_BAD_ARGUMENT;
        PFHE_REQUIRE_ALIGNED(table);
        PFHE_REQUIRE_ALIGNED(selectors);
        PFHE_REQUIRE_ALIGNED(out);
        if (overlaps(table, len_table * sizeof(W), out, len_out * sizeof(W)) ||
            overlaps(selectors, len_selectors * sizeof(double2), out, len_out * sizeof(W))) {
            set_last_error("TFHE CMUX tree: the output must not overlap an input");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    const u32 d = h->depth;
    const size_t glwe = h->glwe;
    const StageBuf bufs[] = {stage_in(table, len_table * sizeof(W)), stage_in(selectors, len_selectors * sizeof(double2)),
                             stage_out(out, len_out * sizeof(W))};
    return handle_call(h->guard, h->fft->device, form, bufs, s, [&](void *const *p, hipStream_t st) -> int {
        const W *leaves = (const W *)p[0];
        // chunk after chunk; every level of a chunk is queued before the next chunk starts
        for (u64 done = 0; done < batch; done += h->chunk) {
            const u64 cur = std::min<u64>(h->chunk, batch - done);
            const double2 *keys = (const double2 *)p[1] + done * d * h->key_len;
            const W *src = shared ? leaves : leaves + (done << d) * glwe;
            for (u32 j = 0; j < d; ++j) {
                const u64 per_input = 1ull << (d - 1 - j);
                W *dst = j + 1 == d ? (W *)p[2] + done * glwe : h->node[j & 1];
                const CmuxNodes at{2 * glwe, 0, per_input, (u64)d * h->key_len, j == 0 && shared ? (u32)per_input : 0u};
                PFHE_TRY(cmux_nodes<W>(h, src, src + glwe, keys + j * h->key_len, dst, cur * per_input, at, st));
                src = dst;
            }
        }
        return PFHE_OK;
    });
}

template <class H>
size_t cmux_scratch(const H *h) {
    return h && h->fft ? h->bufs.bytes() + (h->plan ? h->plan->scratch.bytes() : 0) : 0;
}

}  // namespace

// ---------------- what the look-up handle (pfhe_lut.hip) runs of this file, declared in pfhe_tfhe_handles.hpp ----------------

namespace pfhe {

template <class W>
int tfhe_cmux_core_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t depth,
                          size_t chunk, TfheCmuxTreeCore<W> **out) {
    return cmux_tree_create<W>(fft, glwe_dimension, log_basis, decompose_length, depth, chunk, out);
}

template <class W>
int tfhe_cmux_launch(TfheCmuxTreeCore<W> *h, const W *d0, const W *d1, const double2 *keys, W *out, u64 count,
                     const CmuxSources &at, hipStream_t s) {
    return cmux_nodes<W>(h, d0, d1, keys, out, count, CmuxNodes{at.stride, 0, at.per_key, at.key_stride, at.period}, s);
}

template int tfhe_cmux_core_create<u32>(const pfhe_fft *, size_t, uint32_t, size_t, size_t, size_t, TfheCmuxTreeCore<u32> **);
template int tfhe_cmux_core_create<u64>(const pfhe_fft *, size_t, uint32_t, size_t, size_t, size_t, TfheCmuxTreeCore<u64> **);
template int tfhe_cmux_launch<u32>(TfheCmuxTreeCore<u32> *, const u32 *, const u32 *, const double2 *, u32 *, u64,
                                   const CmuxSources &, hipStream_t);
template int tfhe_cmux_launch<u64>(TfheCmuxTreeCore<u64> *, const u64 *, const u64 *, const double2 *, u64 *, u64,
                                   const CmuxSources &, hipStream_t);

}  // namespace pfhe

// The entry points of one word width.  P: pfhe_tfhe / pfhe_tfhe32; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_CMUX_FAMILY(P, CW, W)                                                                                    \
    PFHE_ENTRY(P##_cmux_tree_create, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                 \
                size_t decompose_length, size_t depth, size_t chunk, P##_cmux_tree_handle **out),                     \
               cmux_tree_create<W>(fft, glwe_dimension, log_basis, decompose_length, depth, chunk, out))              \
    PFHE_HANDLE_TRIO(P##_cmux_tree, P##_cmux_tree_handle, cmux_scratch(h))                                            \
    PFHE_ENTRY(P##_cmux_dev, (P##_cmux_tree_handle *h, const CW *d0_dev, size_t len_d0, const CW *d1_dev,             \
                size_t len_d1, const double *keys_dev, size_t len_keys, size_t per_key, CW *out_dev, size_t len_out,  \
                void *stream),                                                                                        \
               cmux<W>(Form::kDevice, h, (const W *)d0_dev, len_d0, (const W *)d1_dev, len_d1, keys_dev, len_keys,    \
                       per_key, (W *)out_dev, len_out, (hipStream_t)stream))                                          \
    PFHE_ENTRY(P##_cmux, (P##_cmux_tree_handle *h, const CW *d0, size_t len_d0, const CW *d1, size_t len_d1,          \
                const double *keys, size_t len_keys, size_t per_key, CW *out, size_t len_out),                        \
               cmux<W>(Form::kHost, h, (const W *)d0, len_d0, (const W *)d1, len_d1, keys, len_keys, per_key,         \
                       (W *)out, len_out, nullptr))                                                                   \
    PFHE_ENTRY(P##_cmux_tree_dev, (P##_cmux_tree_handle *h, const CW *table_dev, size_t len_table,                    \
                const double *selectors_dev, size_t len_selectors, CW *out_dev, size_t len_out, void *stream),        \
               cmux_tree<W>(Form::kDevice, h, (const W *)table_dev, len_table, selectors_dev, len_selectors,          \
                            (W *)out_dev, len_out, (hipStream_t)stream))                                              \
    PFHE_ENTRY(P##_cmux_tree, (P##_cmux_tree_handle *h, const CW *table, size_t len_table, const double *selectors,   \
                size_t len_selectors, CW *out, size_t len_out),                                                       \
               cmux_tree<W>(Form::kHost, h, (const W *)table, len_table, selectors, len_selectors, (W *)out, len_out, \
                            nullptr))

extern "C" {

PFHE_CMUX_FAMILY(pfhe_tfhe, uint64_t, u64)
PFHE_CMUX_FAMILY(pfhe_tfhe32, uint32_t, u32)
#undef PFHE_CMUX_FAMILY

}  // extern "C"
