// pfhe_ring_pack.hip — ring packing of LWE ciphertexts by automorphisms: the merge of two GLWE ciphertexts and the pack of
// `count` LWE ciphertexts into one GLWE ciphertext built from it (include/pfhe.h: pfhe_ringpack{,32}_*,
// a prefix of its own as pfhe_bitext{,32}_*).  No reference counterpart; DESIGN.md §28 states the rules, §21 the automorphism
// (rule 1), the trace, their keys and the embedding they are made of.
//
//   rule A, the merge   level l in 1..log N, s = N / 2^l, t = 2^l + 1:
//                    D = even - X^s odd, S = even + X^s odd, out = S + automorphism(D, key, t): word for word
//                    mul_monomial_each_to, a wrapping subtraction and addition, rule 1 of §21 and a wrapping addition
//   rule B, the pack    m = ceil(log2 count); node_0[i] = embedding of LWE i (all zero for count <= i < 2^m);
//                    node_l[r] = merge(node_{l-1}[r], node_{l-1}[r + 2^(m-l)], keys[log N - l], level l), l = 1..m;
//                    out = trace(node_m[0], keys[0 .. log N - m), log N - m steps): the phase of LWE i, times N, arrives
//                    at coefficient i N / 2^m
//   fused   (k = 1, N <= 2^11): tfhe_ring_merge_kernel, one launch per level and chunk, a workgroup per node.  D is formed
//            in LDS behind the digit spectrum (the leaves of level 1 are read through the embedding's index rule and never
//            stored), then the trace loop's step: sigma_t(D) gathered into registers, S = 2 even - D at the thread's own
//            slots, the product's accumulate code on the ONE mask row, its inverse code with the accumulating sink.  The
//            root goes on in the same workgroup with the log N - m trailing trace steps;
//   general (every other shape): per level a prepare launch that writes D and S of every node, then the trace's general step
//            on D accumulating into S; then the trace's general steps.  The slow form.
// Nodes live node-major in ONE buffer the handle owns: node r of the chunk's group g is ciphertext r * cur + g.  A level of
// `nodes` nodes per group reads ciphertexts b and b + nodes * cur and writes b, b < nodes * cur: no workgroup writes what
// another reads, and a workgroup reads its two children wholly before its final store, so the update is in place.
#include <algorithm>
#include <cstdint>
#include <memory>

#include "pfhe_tfhe_handles.hpp"
#include "pfhe_trace_device.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// Where the workgroups (fused) or threads (general) of one merge launch find their children.  Item b of the launch is node
// r = b / groups of group g = b mod groups; its even child is item g * group_stride + r * item_stride of `even`, its odd
// child the item odd_offset * item_stride further on in `odd`, absent (all zero) when r + odd_offset >= present.
//   nodes of the node buffer   group_stride 1, item_stride groups, item_words (k+1) N
//   LWE leaves                 group_stride count, item_stride 1, item_words k N + 1, leaves set
//   rule A                     groups = batch, item_stride 0, odd_offset 0, present 1
// single: there is no odd child and no merge (count = 1): the node is the even child itself.
struct MergeSources {
    u32 group_stride, item_stride, item_words, groups, odd_offset, present, leaves, single, level;
};

// word i of polynomial c (c = k: the body) of a child: a GLWE ciphertext as it lies, or an LWE ciphertext through the
// embedding's index rule (rule 4 of §21): A_j[0] = a[jN], A_j[N - i] = -a[jN + i], B = (b, 0, .., 0)
template <class W>
__device__ __forceinline__ W child_word(const W *p, bool leaf, u32 c, u32 i, u32 n, u32 k) {
    if (!leaf) return p[(u64)c * n + i];
    if (c == k) return i == 0 ? p[(u64)k * n] : (W)0;
    return i == 0 ? p[(u64)c * n] : (W)0 - p[(u64)c * n + (n - i)];
}

// One step on the LDS-resident ACC `a` (2N words behind the digit spectrum lds_t), the trace loop's: sigma_t(ACC_A) and
// sigma_t(ACC_B) gathered into registers, a barrier, the body row's sigma_t(ACC_B) added at the thread's own slots, the
// product's accumulate code on the ONE mask row against `key`, its inverse code and the sink ACC -= to_torus(E).  When merging,
// between the barrier and the body's addition ACC becomes 2 even - ACC at the thread's own slots, which turns D into S; even
// is read again from memory there (held in registers across the product it would have to be picked by a run-time slot
// number), one slot at a time so that few loads are in flight at once.
template <class W, bool LEAF>
__device__ __forceinline__ void ring_step(W *a, double2 *lds_t, const W *ev, bool merging, u32 t, const double2 *__restrict__ key,
                                          const double2 *__restrict__ tw, const Shape s) {
    const u32 n = 1u << s.log_n, m = n >> 1;
    const u32 t_inv = odd_inverse(t, 2 * n - 1);
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
    __syncthreads();  // every gather of the step is done: ACC can change at the thread's own slots
    if (merging) {    // S = even + X^s odd = 2 even - D
#pragma unroll 1
        for (u32 i = threadIdx.x; i < m; i += kThreads) {  // the thread's own slots, as the sink's
            a[i] = 2 * child_word(ev, LEAF, 0u, i, n, 1u) - a[i];
            a[i + m] = 2 * child_word(ev, LEAF, 0u, i + m, n, 1u) - a[i + m];
            a[n + i] = 2 * child_word(ev, LEAF, 1u, i, n, 1u) - a[n + i];
            a[n + i + m] = 2 * child_word(ev, LEAF, 1u, i + m, n, 1u) - a[n + i + m];
        }
    }
#pragma unroll
    for (int u = 0; u < kFusedPer; ++u) {
        const u32 i = threadIdx.x + u * kThreads;
        if (i < m) {
            a[n + i] += body_lo[u];
            a[n + i + m] += body_hi[u];
        }
    }
    fused_accumulate_rows<W, 1>([&](u32) { return mask; }, ClassicKey{key}, lds_t, tw, s, acc0, acc1);
    fused_inverse_rows(acc0, acc1, lds_t, tw, s, [&](u32 c, u32 i, double lo, double hi) {
        a[c * n + i] -= to_torus<W>(lo);
        a[c * n + i + m] -= to_torus<W>(hi);
    });
}

// One node per workgroup (k = 1, N <= 2^11): ACC (2N words) sits in LDS behind the digit spectrum, as in
// tfhe_trace_loop_kernel.  The prologue writes D = even - X^s odd into ACC (X^s is an index shift with a sign; an absent
// child reads as zero; with `single` ACC is the one child and the merge step is skipped).  The merge step is the trace
// loop's: sigma_t(D_A) and sigma_t(D_B) gathered from ACC into registers, a barrier, then at the thread's own slots
// ACC = 2 even - ACC, which is S, plus sigma_t(D_B) on the body row (even is read again from memory: held in registers
// across the product it would have to be picked by a run-time slot number), the product's accumulate code on the mask row
// against the level's key, its inverse code and the sink ACC -= to_torus(E).  `tail` are the trailing trace steps of the
// root, the trace loop's step unchanged, against keys[0 .. tail.count).  Both children are read wholly before the one
// store loop at the end, so out may be exactly even.  (No __restrict__ on the three for that reason.)
template <class W, bool LEAF>
__global__ __launch_bounds__(kThreads) void tfhe_ring_merge_kernel(const W *even, const W *odd, const double2 *__restrict__ keys,
                                                                   u32 merge_key, W *out, MergeSources src, TraceSteps tail,
                                                                   const double2 *__restrict__ tw, Shape s) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_t[];
    const u32 n = 1u << s.log_n;
    W *a = reinterpret_cast<W *>(reinterpret_cast<char *>(lds_t) + lds_bytes(s.log_n));
    const u32 r = blockIdx.x / src.groups, g = blockIdx.x - r * src.groups;
    const bool merge = src.single == 0;
    const W *ev = even + ((u64)g * src.group_stride + (u64)r * src.item_stride) * src.item_words;
    const bool has_odd = merge && r + src.odd_offset < src.present;
    const W *od = odd + ((u64)g * src.group_stride + (u64)(r + src.odd_offset) * src.item_stride) * src.item_words;
    W *o = out + (u64)blockIdx.x * 2 * n;
    const MonomialShift shift(merge ? n >> src.level : 0u, n);
    for (u32 x = threadIdx.x; x < 2 * n; x += blockDim.x) {
        const u32 c = x >> s.log_n, i = x & (n - 1);
        W v = child_word(ev, LEAF, c, i, n, 1u);
        if (has_odd) v -= shift.apply(i, child_word(od, LEAF, c, shift.source(i), n, 1u));
        a[x] = v;
    }
    __syncthreads();
    const u64 key_len = (u64)2 * s.ell * n;
    const u32 first = merge ? 1u : 0u;
    for (u32 step = 0; step < first + tail.count; ++step) {
        const bool merging = step < first;
        ring_step<W, LEAF>(a, lds_t, ev, merging, merging ? (1u << src.level) + 1 : tail.t[step - first],
                     keys + (merging ? merge_key : step - first) * key_len, tw, s);
    }
    for (u32 i = threadIdx.x; i < 2 * n; i += blockDim.x) o[i] = a[i];
}

// The general form's prepare, one thread per word of the launch's nodes: D = even - X^s odd goes to d, S = even + X^s odd to
// sum (with `single`, the one child to sum and nothing to d).  A thread reads even at its own index alone, so sum may be
// exactly even when the children are nodes.
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_ring_prepare_kernel(const W *even, const W *odd, W *__restrict__ d, W *sum,
                                                                     MergeSources src, u32 log_n, u32 k, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n, i = (u32)(t & (n - 1));
    const u64 poly = t >> log_n, b = poly / (k + 1);
    const u32 c = (u32)(poly - b * (k + 1));
    const u32 r = (u32)(b / src.groups), g = (u32)(b - (u64)r * src.groups);
    const bool leaf = src.leaves != 0;
    const W *ev = even + ((u64)g * src.group_stride + (u64)r * src.item_stride) * src.item_words;
    const W v = child_word(ev, leaf, c, i, n, k);
    if (src.single) {
        sum[t] = v;
        return;
    }
    W w = 0;
    if (r + src.odd_offset < src.present) {
        const W *od = odd + ((u64)g * src.group_stride + (u64)(r + src.odd_offset) * src.item_stride) * src.item_words;
        const MonomialShift shift(n >> src.level, n);
        w = shift.apply(i, child_word(od, leaf, c, shift.source(i), n, k));
    }
    d[t] = v - w;
    sum[t] = v + w;
}

}  // namespace
}  // namespace pfhe

// ---------------- the handle ----------------

// Owns the node buffer of chunk * max(1, 2^(M-1)) ciphertexts, M = ceil(log2 max_count), and off the fused shape a trace
// core sized for as many ciphertexts (the general step's buffers and the product's scratch) and the D buffer.  All
// allocated at creation.
template <class W>
struct TfheRingPackCore {
    const pfhe_fft *fft = nullptr;  // borrowed (must outlive the handle)
    PlanGuard guard;                // one holder at a time, successive calls on different streams ordered
    Shape shape{};
    bool fused = false;
    size_t chunk = 1, glwe = 0, lwe = 0, key_len = 0, max_count = 1, cap = 1;  // cap: nodes of a group after level 1, at most
    std::unique_ptr<TfheTraceCore<W>> core;                                    // owned, general form only
    W *nodes = nullptr, *d = nullptr;
    DeviceBuffers bufs;  // after the core: the two buffers are freed first
};
struct pfhe_ringpack : TfheRingPackCore<u64> {};
struct pfhe_ringpack32 : TfheRingPackCore<u32> {};

namespace {

constexpr const char *kRingBusy = "TFHE ring-packing handle in use by another thread (one handle per thread)";
constexpr size_t kRingDefaultBytes = 256ull << 20;

u32 ceil_log2(size_t v) {
    u32 m = 0;
    while (((size_t)1 << m) < v) ++m;
    return m;
}

// the product plan's checks in their order, the dimension, then max_count, all before the device; then every allocation
template <class W, class H>
int ring_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t max_count,
                size_t chunk, H **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    Shape sh{};
    PFHE_TRY(tfhe_plan_check<W>(fft, glwe_dimension, log_basis, decompose_length, sh));
    if (glwe_dimension == 0) {
        set_last_error("TFHE ring packing: glwe_dimension must be at least 1");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (max_count == 0 || max_count > fft->n) {
        set_last_error("TFHE ring packing: max_count must be in 1..N");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    auto h = std::make_unique<H>();
    h->shape = sh;
    h->fused = sh.k == 1 && sh.log_n <= kFusedMaxLogN;
    h->glwe = (glwe_dimension + 1) * fft->n;
    h->lwe = glwe_dimension * fft->n + 1;
    h->key_len = glwe_dimension * sh.ell * h->glwe;
    h->max_count = max_count;
    const u32 big_m = ceil_log2(max_count);
    h->cap = big_m ? (size_t)1 << (big_m - 1) : 1;
    // the default chunk: the node buffer, and off the fused shape the general step's buffers and spectra, near 256 MiB
    size_t per_node = h->glwe * sizeof(W);
    if (!h->fused) per_node += 3 * h->glwe * sizeof(W) + (glwe_dimension + 1) * (sh.ell + 1) * (fft->n / 2) * sizeof(double2);
    h->chunk = chunk ? chunk : std::max<size_t>(1, kRingDefaultBytes / (per_node * h->cap));
    h->chunk = std::min<size_t>(h->chunk, 0x7fffffffull / (h->cap * (glwe_dimension + 1) * sh.ell));  // a launch's grid
    if (h->chunk == 0) {
        set_last_error("TFHE ring packing: max_count nodes of this shape exceed one launch");
        return PFHE_ERR_UNSUPPORTED;
    }
    DeviceGuard g(fft->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    h->fft = fft;
    if (!h->fused) {
        TfheTraceCore<W> *core = nullptr;
        PFHE_TRY(tfhe_trace_core_create<W>(fft, glwe_dimension, log_basis, decompose_length, h->chunk * h->cap, &core));
        h->core.reset(core);
        if (core->chunk < h->chunk * h->cap) {
            set_last_error("TFHE ring packing: chunk * max_count nodes exceed one launch of the general form");
            return PFHE_ERR_UNSUPPORTED;
        }
    }
    h->bufs.bind(fft->device);
    PFHE_TRY(h->bufs.add(h->nodes, h->chunk * h->cap * h->glwe));
    if (!h->fused) PFHE_TRY(h->bufs.add(h->d, h->chunk * h->cap * h->glwe));
    PFHE_TRY(h->guard.init(fft->device));
    *out = h.release();
    return PFHE_OK;
}

// One level on `items` nodes (items = src.groups * nodes of a group): the children as src finds them, the result to `out`
// node-major, which may be where the even children lie.  tail: the root's trailing trace steps (keys[0 .. tail.count)).
template <class W>
int merge_level(TfheRingPackCore<W> *h, const W *even, const W *odd, const double2 *keys, u32 merge_key, W *out, u64 items,
                const MergeSources &src, const TraceSteps &tail, hipStream_t s) {
    const pfhe_fft &f = *h->fft;
    if (h->fused)
        return launch_groups(src.leaves ? tfhe_ring_merge_kernel<W, true> : tfhe_ring_merge_kernel<W, false>, items,
                             lds_bytes(f.log_n) + 2 * f.n * sizeof(W), s, even, odd, keys, merge_key, out, src, tail, f.tw, h->shape);
    PFHE_TRY(launch_flat(tfhe_ring_prepare_kernel<W>, items * h->glwe, s, even, odd, h->d, out, src, f.log_n, h->shape.k));
    if (!src.single)
        PFHE_TRY(tfhe_trace_general_step<W>(h->core.get(), (const W *)h->d, (const W *)out, out, keys + (u64)merge_key * h->key_len,
                                            (1u << src.level) + 1, 1u, items, s));
    if (tail.count) PFHE_TRY(tfhe_trace_steps<W>(h->core.get(), (const W *)out, keys, out, items, tail, s));
    return PFHE_OK;
}

// rule A on `batch` pairs, chunk after chunk
template <class W>
int merge_launches(TfheRingPackCore<W> *h, const W *even, const W *odd, const double2 *key, W *out, u64 batch, u32 level,
                   hipStream_t s) {
    for (u64 done = 0; done < batch; done += h->chunk) {
        const u64 cur = std::min<u64>(h->chunk, batch - done);
        const MergeSources src{1, 0, (u32)h->glwe, (u32)cur, 0, 1, 0, 0, level};
        PFHE_TRY(merge_level<W>(h, even + done * h->glwe, odd + done * h->glwe, key, 0, out + done * h->glwe, cur, src, TraceSteps{}, s));
    }
    return PFHE_OK;
}

// rule B on `batch` groups of `count` LWE ciphertexts, chunk after chunk, every level of a chunk queued before the next
// chunk starts
template <class W>
int pack_launches(TfheRingPackCore<W> *h, const W *lwe, const double2 *keys, W *out, u64 batch, u32 count, hipStream_t s) {
    const u32 log_n = h->fft->log_n, m = ceil_log2(count);
    TraceSteps tail{log_n - m, 1, {}};
    for (u32 st = 1; st <= tail.count; ++st) tail.t[st - 1] = (1u << (log_n - st + 1)) + 1;
    const TraceSteps none{};
    for (u64 done = 0; done < batch; done += h->chunk) {
        const u32 cur = (u32)std::min<u64>(h->chunk, batch - done);
        const W *x = lwe + done * count * h->lwe;
        W *o = out + done * h->glwe;
        if (m == 0) {
            const MergeSources src{1, 0, (u32)h->lwe, cur, 0, 1, 1, 1, 0};
            PFHE_TRY(merge_level<W>(h, x, x, keys, 0, o, cur, src, tail, s));
            continue;
        }
        for (u32 level = 1; level <= m; ++level) {
            const u32 nodes = 1u << (m - level);
            const bool root = level == m;
            W *dst = root ? o : h->nodes;
            const MergeSources src = level == 1 ? MergeSources{count, 1, (u32)h->lwe, cur, nodes, count, 1, 0, level}
                                                : MergeSources{1, cur, (u32)h->glwe, cur, nodes, 2 * nodes, 0, 0, level};
            const W *in = level == 1 ? x : h->nodes;
            PFHE_TRY(merge_level<W>(h, in, in, keys, log_n - level, dst, (u64)cur * nodes, src, root ? tail : none, s));
        }
    }
    return PFHE_OK;
}

template <class W>
int ring_merge(Form form, TfheRingPackCore<W> *h, const W *even, size_t len_even, const W *odd, size_t len_odd, const double *key,
               size_t len_key, uint32_t level, W *out, size_t len_out, hipStream_t s) {
    if (!h || !h->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kRingBusy);
    if (level == 0 || level > h->fft->log_n) {
        set_last_error("TFHE ring merge: level must be in 1..log N");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (form == Form::kHost && ((!even && len_even) || (!odd && len_odd) || (!key && len_key) || (!out && len_out)))
        return PFHE_ERR_BAD_ARGUMENT;
    if (len_even % h->glwe != 0 || len_odd != len_even || len_out != len_even || len_key != h->key_len) {
        set_last_error("TFHE ring merge: even, odd and out must be batch*(k+1)*N words and the key k*ell*(k+1)*N complex values");
        return PFHE_ERR_BAD_LENGTH;
    }
    const u64 batch = len_even / h->glwe;
    if (batch == 0) return PFHE_OK;
    if (form == Form::kDevice) {
        if (!even || !odd || !key || !out) return PFHE_ERR_BAD_ARGUMENT;
        PFHE_REQUIRE_ALIGNED(even);
        PFHE_REQUIRE_ALIGNED(odd);
        PFHE_REQUIRE_ALIGNED(key);
        PFHE_REQUIRE_ALIGNED(out);
        const size_t bytes = len_out * sizeof(W);
        // a node reads both children wholly before it writes, and writes where its even child lies
        if ((even != out && overlaps(even, bytes, out, bytes)) || overlaps(odd, bytes, out, bytes) ||
            overlaps(key, len_key * sizeof(double2), out, bytes)) {
            set_last_error("TFHE ring merge: out must be exactly even or disjoint from it, and disjoint from odd and the key");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    const StageBuf bufs[] = {stage_in(even, len_even * sizeof(W)), stage_in(odd, len_odd * sizeof(W)),
                             stage_in(key, len_key * sizeof(double2)), stage_out(out, len_out * sizeof(W))};
    return handle_call(h->guard, h->fft->device, form, bufs, s, [&](void *const *p, hipStream_t st) {
        return merge_launches<W>(h, (const W *)p[0], (const W *)p[1], (const double2 *)p[2], (W *)p[3], batch, level, st);
    });
}

template <class W>
int ring_pack(Form form, TfheRingPackCore<W> *h, const W *lwe, size_t len_lwe, const double *keys, size_t len_keys, size_t count,
              W *out, size_t len_out, hipStream_t s) {
    if (!h || !h->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kRingBusy);
    if (count == 0 || count > h->max_count) {
        set_last_error("TFHE ring pack: count must be in 1..max_count");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (form == Form::kHost && ((!lwe && len_lwe) || (!keys && len_keys) || (!out && len_out))) return PFHE_ERR_BAD_ARGUMENT;
    const size_t group = count * h->lwe;
    if (len_lwe % group != 0 || len_out != len_lwe / group * h->glwe || len_keys != h->fft->log_n * h->key_len) {
        set_last_error("TFHE ring pack: lwe_in must be batch*count*(k*N+1) words, glwe_out batch*(k+1)*N words and keys "
                       "log N*k*ell*(k+1)*N complex values");
        return PFHE_ERR_BAD_LENGTH;
    }
    const u64 batch = len_lwe / group;
    if (batch == 0) return PFHE_OK;
    if (form == Form::kDevice) {
        if (!lwe || !keys || !out) return PFHE_ERR_BAD_ARGUMENT;
        PFHE_REQUIRE_ALIGNED(lwe);
        PFHE_REQUIRE_ALIGNED(keys);
        PFHE_REQUIRE_ALIGNED(out);
        const size_t bytes = len_out * sizeof(W);
        if (overlaps(lwe, len_lwe * sizeof(W), out, bytes) || overlaps(keys, len_keys * sizeof(double2), out, bytes)) {
            set_last_error("TFHE ring pack: glwe_out must overlap neither lwe_in nor the keys");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    const StageBuf bufs[] = {stage_in(lwe, len_lwe * sizeof(W)), stage_in(keys, len_keys * sizeof(double2)),
                             stage_out(out, len_out * sizeof(W))};
    return handle_call(h->guard, h->fft->device, form, bufs, s, [&](void *const *p, hipStream_t st) {
        return pack_launches<W>(h, (const W *)p[0], (const double2 *)p[1], (W *)p[2], batch, (u32)count, st);
    });
}

template <class H>
size_t ring_scratch(const H *h) {
    return h->fft ? h->bufs.bytes() + (h->core ? h->core->bufs.bytes() + h->core->scratch.bytes() : 0) : 0;
}

}  // namespace

// The entry points of one word width.  P: pfhe_ringpack / pfhe_ringpack32, the family's own prefix and its handle type; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_RING_PACK_FAMILY(P, CW, W)                                                                                   \
    PFHE_ENTRY(P##_create, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                     \
                size_t decompose_length, size_t max_count, size_t chunk, P **out),                     \
               ring_create<W>(fft, glwe_dimension, log_basis, decompose_length, max_count, chunk, out))                   \
    PFHE_HANDLE_TRIO(P, P, ring_scratch(h))                                                \
    PFHE_ENTRY(P##_merge_dev, (P *h, const CW *even_dev, size_t len_even, const CW *odd_dev, \
                size_t len_odd, const double *key_dev, size_t len_key, uint32_t level, CW *out_dev, size_t len_out,       \
                void *stream),                                                                                            \
               ring_merge<W>(Form::kDevice, h, (const W *)even_dev, len_even, (const W *)odd_dev, len_odd, key_dev,       \
                             len_key, level, (W *)out_dev, len_out, (hipStream_t)stream))                                 \
    PFHE_ENTRY(P##_merge, (P *h, const CW *even, size_t len_even, const CW *odd,             \
                size_t len_odd, const double *key, size_t len_key, uint32_t level, CW *out, size_t len_out),              \
               ring_merge<W>(Form::kHost, h, (const W *)even, len_even, (const W *)odd, len_odd, key, len_key, level,     \
                             (W *)out, len_out, nullptr))                                                                 \
    PFHE_ENTRY(P##_pack_dev, (P *h, const CW *lwe_dev, size_t len_lwe,                        \
                const double *keys_dev, size_t len_keys, size_t count, CW *glwe_out_dev, size_t len_out, void *stream),   \
               ring_pack<W>(Form::kDevice, h, (const W *)lwe_dev, len_lwe, keys_dev, len_keys, count, (W *)glwe_out_dev,  \
                            len_out, (hipStream_t)stream))                                                                \
    PFHE_ENTRY(P##_pack, (P *h, const CW *lwe, size_t len_lwe, const double *keys,            \
                size_t len_keys, size_t count, CW *glwe_out, size_t len_out),                                             \
               ring_pack<W>(Form::kHost, h, (const W *)lwe, len_lwe, keys, len_keys, count, (W *)glwe_out, len_out,       \
                            nullptr))

extern "C" {

PFHE_RING_PACK_FAMILY(pfhe_ringpack, uint64_t, u64)
PFHE_RING_PACK_FAMILY(pfhe_ringpack32, uint32_t, u32)
#undef PFHE_RING_PACK_FAMILY

}  // extern "C"
