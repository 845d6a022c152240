// pfhe_lut.hip — a look-up table of 2^p entries evaluated on p encrypted bits: a CMUX tree over the high bits (vertical
// packing), a rotation by the low bits (horizontal packing), sample extraction (include/pfhe.h: pfhe_tfhe{,32}_lut_*,
// _rotate_by_bits*, _lut_eval*).  No reference counterpart; DESIGN.md §23 states the rules.  Built on the arithmetic of
// external_product_to (pfhe_fft.hip) and on the CMUX (pfhe_cmux.hip), which stay what they are.
//
//   rule 1, the rotation  acc_0 = inp[a], acc_{j+1} = acc_j + external_product_to(X^{2N - 2^(j+s)} acc_j - acc_j, key_j(a)),
//                         j = 0..r-1, out[a] = acc_r, key_j(a) = keys[(a / o) keys_per_input + first_key + j]: per step the
//                         words of mul_monomial_each_to_dev, then the CMUX with d0 = acc, d1 = the rotated one, per_key = o.
//   rule 2, the table     stage A, the tree of §20 on the nodes (input, output, leaf) with bit r + j at level j; stage B, rule 1
//                         on its batch * o results (on the table itself at tree depth 0); stage C, sample extraction at the
//                         indices below `extract` (launch_extract on the stored ciphertexts), or none.
//   fused   (k = 1, N <= 2^11): tfhe_bitrot_loop_kernel, ONE launch per chunk for all r steps, a workgroup per accumulator,
//            ACC in LDS from the first step to the last; the tree's levels are tfhe_cmux_kernel launches (tfhe_cmux_launch).
//   general (every other shape): per step tfhe_bitrot_monomial_kernel into an owned buffer, then the CMUX's general form in
//            place.  Correct and slow.
// Nothing is atomic and the summation order is the product's: the words depend neither on the batch nor on the chunk.
#include <algorithm>
#include <cstdint>
#include <memory>

#include "pfhe_tfhe_exact_device.hpp"
#include "pfhe_tfhe_handles.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// Where a launch of the rotation finds its accumulators and keys.  Accumulator b of the launch (blockIdx.x) has the global
// index first_acc + b: it reads its input at (period ? (first_acc + b) mod period : b) ciphertexts from `in` (a period is
// the shared table of a tree of depth 0), writes out at b, and its key of step j is keys + ((first_acc + b) / per_input) *
// key_stride + j * key_len: a chunk boundary inside an input's outputs still picks the input's keys.
struct BitRot {
    u64 first_acc, per_input, key_stride;
    u32 period, steps, log_stride;
    __device__ __forceinline__ u64 source(u64 b) const { return period ? (first_acc + b) % period : b; }
    __device__ __forceinline__ u64 key(u64 b) const { return ((first_acc + b) / per_input) * key_stride; }
    // the exponent of step j, 2N - 2^(j + s): X^{-2^(j+s)}
    __device__ __host__ __forceinline__ u32 exponent(u32 j, u32 n) const { return 2 * n - (1u << (j + log_stride)); }
};

// All r steps of one accumulator in one workgroup (k = 1, N <= 2^11): ACC (2N words) sits in LDS behind the digit spectrum
// from the first step to the last, as in tfhe_blindrot_loop_kernel, but the key of a step is the accumulator's own.  The
// input is read wholly into LDS, behind a barrier, before anything is written: out may be exactly in.  Per step: D row by
// row from the LDS-resident ACC into registers, the product's own accumulate and inverse code against the step's key, ACC
// += E in LDS.  Every gather of a step precedes a barrier of fused_accumulate_rows, every update follows the barrier that
// ends it, each thread updates the words it alone owns, and fused_inverse_rows ends behind a barrier, so no step reads a
// word the same step has already updated and the next step's gathers see every update.  (No __restrict__ on in / out.)
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_bitrot_loop_kernel(const W *in, const double2 *__restrict__ keys, W *out,
                                                                    const double2 *__restrict__ tw, Shape s, BitRot at) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_b[];
    const u32 n = 1u << s.log_n, m = n >> 1;
    W *a = reinterpret_cast<W *>(reinterpret_cast<char *>(lds_b) + lds_bytes(s.log_n));
    const W *g = in + at.source(blockIdx.x) * 2 * n;
    for (u32 i = threadIdx.x; i < 2 * n; i += blockDim.x) a[i] = g[i];
    __syncthreads();
    const u64 key_len = (u64)4 * s.ell * n;
    const double2 *key0 = keys + at.key(blockIdx.x);
    for (u32 step = 0; step < at.steps; ++step) {
        const MonomialShift x(at.exponent(step, n), n);
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
        }, ClassicKey{key0 + step * key_len}, lds_b, tw, s, acc0, acc1);
        fused_inverse_rows(acc0, acc1, lds_b, tw, s, [&](u32 c, u32 i, double lo, double hi) {
            a[c * n + i] += to_torus<W>(lo);
            a[c * n + i + m] += to_torus<W>(hi);
        });
    }
    W *o = out + (u64)blockIdx.x * 2 * n;
    for (u32 i = threadIdx.x; i < 2 * n; i += blockDim.x) o[i] = a[i];
}

// The general form's rotation, one thread per word of `glwe` words per accumulator: out = X^e in on every polynomial, the
// words of mul_monomial_each_to_dev with the one exponent e for all (e = 0: a copy, which gathers a shared table).  out
// must not overlap in.
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_bitrot_monomial_kernel(const W *__restrict__ in, W *__restrict__ out, u32 e,
                                                                        u32 log_n, u64 glwe, BitRot at, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n;
    const u64 b = t / glwe, w = t - b * glwe;
    const u32 j = (u32)(w & (n - 1));
    const MonomialShift x(e, n);
    const W *p = in + at.source(b) * glwe + (w - j);
    out[t] = x.apply(j, p[x.source(j)]);
}

}  // namespace
}  // namespace pfhe

// ---------------- the handle ----------------

// Owns, for `chunk` inputs of `outputs` look-ups each: one buffer of chunk * o ciphertexts (the rotation's accumulators when
// the call extracts), in the general form a second one (the rotated accumulators), and, with a tree or in the general form,
// a CMUX core for chunk * o inputs of a tree of depth max(t, 1): its node buffers, and off the fused shape its product plan
// and D and E buffers.  All allocated at creation.
template <class W>
struct TfheLutCore {
    const pfhe_fft *fft = nullptr;  // borrowed (must outlive the handle)
    PlanGuard guard;                // one holder at a time, successive calls on different streams ordered
    Shape shape{};
    u32 t = 0, r = 0, log_stride = 0;
    bool fused = false;
    size_t outputs = 1, chunk = 1, glwe = 0, key_len = 0;
    std::unique_ptr<TfheCmuxTreeCore<W>> tree;  // owned: t > 0 or the general form
    W *acc = nullptr, *rot = nullptr;
    DeviceBuffers bufs;  // after the tree: the two buffers are freed first, then the tree
    size_t bits() const { return (size_t)t + r; }
};
struct pfhe_tfhe_lut_handle : TfheLutCore<u64> {};
struct pfhe_tfhe32_lut_handle : TfheLutCore<u32> {};

namespace {

constexpr const char *kLutBusy = "TFHE look-up handle in use by another thread (one handle per thread)";
constexpr const char *kRotLengths = "TFHE rotation by bits: inp and out must be count*(k+1)*N words, count a multiple of outputs, "
                                    "first_key + rot_bits at most keys_per_input, and keys (count/outputs)*keys_per_input keys "
                                    "of (k+1)*ell*(k+1)*N complex values";
constexpr const char *kLutLengths = "TFHE look-up: out must be batch*outputs ciphertexts of (k+1)*N words, or with extract "
                                    "batch*outputs*extract of k*N+1 words, selectors batch*(tree_depth+rot_bits) keys of "
                                    "(k+1)*ell*(k+1)*N complex values and table outputs*2^tree_depth or batch times as many "
                                    "ciphertexts";
constexpr size_t kLutDefaultBytes = 256ull << 20;
constexpr size_t kLutMaxDepth = 16;

// a null out pointer, the product plan's checks in their order, the four parameters, the grid of a launch, all before the
// device; then every allocation
template <class W, class H>
int lut_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t tree_depth,
               size_t rot_bits, size_t log_stride, size_t outputs, size_t chunk, H **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    Shape sh{};
    PFHE_TRY(tfhe_plan_check<W>(fft, glwe_dimension, log_basis, decompose_length, sh));
    if (tree_depth > kLutMaxDepth) {
        set_last_error("TFHE look-up: tree_depth must be in 0..16");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (rot_bits > sh.log_n || log_stride > sh.log_n - rot_bits) {
        set_last_error("TFHE look-up: rot_bits + log_stride must be at most log N");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (tree_depth + rot_bits == 0) {
        set_last_error("TFHE look-up: tree_depth + rot_bits must be at least 1");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (outputs == 0) {
        set_last_error("TFHE look-up: outputs must be at least 1");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    auto h = std::make_unique<H>();
    h->shape = sh;
    h->t = (u32)tree_depth;
    h->r = (u32)rot_bits;
    h->log_stride = (u32)log_stride;
    h->outputs = outputs;
    h->fused = sh.k == 1 && sh.log_n <= kFusedMaxLogN;
    h->glwe = (glwe_dimension + 1) * fft->n;
    h->key_len = (glwe_dimension + 1) * sh.ell * h->glwe;
    // a launch's grid holds the widest level of the tree, chunk * o * 2^(t-1) nodes, and the chunk * o accumulators
    const size_t depth = std::max<size_t>(1, tree_depth), half = (size_t)1 << (depth - 1);
    const size_t limit = 0x7fffffffull >> (depth - 1);
    if (outputs > limit) return PFHE_ERR_BAD_LENGTH;
    // ciphertexts per input and output: the accumulator, the tree's two node buffers, and in the general form the rotated
    // accumulator and the CMUX's D and E
    const size_t nodes = tree_depth > 1 ? half + half / 2 : 0;
    const size_t per_input = outputs * (1 + nodes + (h->fused ? 0 : 1 + 2 * half));
    h->chunk = chunk ? chunk : std::max<size_t>(1, kLutDefaultBytes / (per_input * h->glwe * sizeof(W)));
    if (h->chunk > limit / outputs) {
        if (chunk) return PFHE_ERR_BAD_LENGTH;
        h->chunk = limit / outputs;
    }
    DeviceGuard g(fft->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    h->fft = fft;
    if (tree_depth > 0 || !h->fused) {
        TfheCmuxTreeCore<W> *tree = nullptr;
        PFHE_TRY(tfhe_cmux_core_create<W>(fft, glwe_dimension, log_basis, decompose_length, depth, h->chunk * outputs, &tree));
        h->tree.reset(tree);
    }
    h->bufs.bind(fft->device);
    PFHE_TRY(h->bufs.add(h->acc, h->chunk * outputs * h->glwe));
    PFHE_TRY(h->bufs.add(h->rot, h->fused ? 0 : h->chunk * outputs * h->glwe));
    PFHE_TRY(h->guard.init(fft->device));
    *out = h.release();
    return PFHE_OK;
}

// Rule 1 on `count` accumulators, at most chunk * o per launch: accumulator a of the call has the global index first + a,
// reads src (by `period`, or at its own index), and ends in dst, which may be exactly src when there is no period.  keys
// points at step 0's key of input 0.  Arguments are checked, the device is current.
template <class W>
int rotate_accs(TfheLutCore<W> *h, const W *src, const double2 *keys, W *dst, u64 first, u64 count, u64 keys_per_input,
                u32 period, hipStream_t s) {
    const pfhe_fft &f = *h->fft;
    const u64 per_launch = (u64)h->chunk * h->outputs, glwe = h->glwe;
    const u32 n = (u32)f.n;
    for (u64 done = 0; done < count; done += per_launch) {
        const u64 cur = std::min<u64>(per_launch, count - done);
        const BitRot at{first + done, (u64)h->outputs, keys_per_input * h->key_len, period, h->r, h->log_stride};
        const W *in = period ? src : src + done * glwe;
        W *o = dst + done * glwe;
        if (h->r == 0) {
            if (in != o) PFHE_HIP(hipMemcpyAsync(o, in, cur * glwe * sizeof(W), hipMemcpyDeviceToDevice, s));
            continue;
        }
        if (h->fused) {
            PFHE_TRY(launch_groups(tfhe_bitrot_loop_kernel<W>, cur, lds_bytes(f.log_n) + glwe * sizeof(W), s, in, keys, o, f.tw,
                                   h->shape, at));
            continue;
        }
        // the general form: the accumulators in dst, gathered from a shared table first; per step the rotated ones into the
        // owned buffer, then the CMUX in place with the step's key of every input
        const W *cur_acc = in;
        if (period) {
            PFHE_TRY(launch_flat(tfhe_bitrot_monomial_kernel<W>, cur * glwe, s, in, o, 0u, f.log_n, glwe, at));
            cur_acc = o;
        }
        BitRot own = at;
        own.period = 0;
        for (u32 j = 0; j < h->r; ++j) {
            PFHE_TRY(launch_flat(tfhe_bitrot_monomial_kernel<W>, cur * glwe, s, cur_acc, h->rot, at.exponent(j, n), f.log_n, glwe,
                                 own));
            // node b of this launch belongs to input (first + done + b) / o: the keys start at the launch's first input, and
            // the launch starts on an input's first output (per_launch and every chunk's first accumulator are multiples of o)
            const double2 *kj = keys + ((first + done) / h->outputs) * at.key_stride + j * h->key_len;
            PFHE_TRY(tfhe_cmux_launch<W>(h->tree.get(), cur_acc, (const W *)h->rot, kj, o, cur,
                                         CmuxSources{glwe, (u64)h->outputs, at.key_stride, 0u}, s));
            cur_acc = o;
        }
    }
    return PFHE_OK;
}

// The host form refuses a null pointer before the lengths; the device form's pointer tests follow the empty batch.
template <class W>
int rotate_by_bits(Form form, TfheLutCore<W> *h, const W *inp, size_t len_inp, const double *keys, size_t len_keys,
                   size_t keys_per_input, size_t first_key, W *out, size_t len_out, hipStream_t s) {
    if (!h || !h->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kLutBusy);
    if (form == Form::kHost && ((!inp && len_inp) || (!keys && len_keys) || (!out && len_out))) return PFHE_ERR_BAD_ARGUMENT;
    const u64 count = len_inp / h->glwe;
    if (len_inp % h->glwe != 0 || len_out != len_inp || count % h->outputs != 0 || first_key > keys_per_input ||
        h->r > keys_per_input - first_key || (keys_per_input && count / h->outputs > SIZE_MAX / keys_per_input / h->key_len) ||
        len_keys != count / h->outputs * keys_per_input * h->key_len) {
        set_last_error(kRotLengths);
        return PFHE_ERR_BAD_LENGTH;
    }
    if (count == 0) return PFHE_OK;
    if (form == Form::kDevice) {
        if (!inp || (!keys && len_keys) || !out) return PFHE_ERR_BAD_ARGUMENT;
        PFHE_REQUIRE_ALIGNED(inp);
        PFHE_REQUIRE_ALIGNED(keys);
        PFHE_REQUIRE_ALIGNED(out);
        // in place is safe (tfhe_bitrot_loop_kernel; the general form rotates into its own buffer and the CMUX adds index by
        // index)
        const size_t bytes = len_out * sizeof(W);
        if ((out != inp && overlaps(inp, bytes, out, bytes)) ||
            (len_keys && overlaps(keys, len_keys * sizeof(double2), out, bytes))) {
            set_last_error("TFHE rotation by bits: out must be exactly inp or disjoint from it, and disjoint from the keys");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    const StageBuf bufs[] = {stage_in(inp, len_inp * sizeof(W)), stage_in(keys, len_keys * sizeof(double2)),
                             stage_out(out, len_out * sizeof(W))};
    return handle_call(h->guard, h->fft->device, form, bufs, s, [&](void *const *p, hipStream_t st) {
        return rotate_accs<W>(h, (const W *)p[0], (const double2 *)p[1] + first_key * h->key_len, (W *)p[2], 0, count,
                              keys_per_input, 0u, st);
    });
}

// batch from the output; the table is shared when it holds o 2^t ciphertexts (at batch 1 the two readings coincide)
template <class W>
bool lut_lengths_ok(const TfheLutCore<W> *h, size_t len_table, size_t len_selectors, size_t len_out, size_t extract, u64 &batch,
                    bool &shared) {
    const size_t k_n = h->glwe - h->fft->n;  // k N
    if (extract && h->outputs > SIZE_MAX / extract / (k_n + 1)) return false;
    const size_t per_input = h->outputs * (extract ? extract * (k_n + 1) : h->glwe);
    if (len_out % per_input != 0) return false;
    batch = len_out / per_input;
    const size_t leaves = (h->glwe * h->outputs) << h->t;
    shared = len_table == leaves;
    if (batch && (batch > SIZE_MAX / leaves || batch > SIZE_MAX / (h->bits() * h->key_len))) return false;
    return len_selectors == batch * h->bits() * h->key_len && (shared || len_table == batch * leaves);
}

// extract above N first; then the refusals of the CMUX tree, in its order
template <class W>
int lut_eval(Form form, TfheLutCore<W> *h, const W *table, size_t len_table, const double *selectors, size_t len_selectors,
             size_t extract, W *out, size_t len_out, hipStream_t s) {
    if (!h || !h->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kLutBusy);
    if (extract > h->fft->n) {
        set_last_error("TFHE look-up: extract must be at most N");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (form == Form::kHost && ((!table && len_table) || (!selectors && len_selectors) || (!out && len_out)))
        return PFHE_ERR_BAD_ARGUMENT;
    u64 batch = 0;
    bool shared = false;
    if (!lut_lengths_ok(h, len_table, len_selectors, len_out, extract, batch, shared)) {
        set_last_error(kLutLengths);
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
            set_last_error("TFHE look-up: the output must not overlap an input");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    const u32 t = h->t, k = h->shape.k;
    const size_t glwe = h->glwe, o = h->outputs, p = h->bits();
    const StageBuf bufs[] = {stage_in(table, len_table * sizeof(W)), stage_in(selectors, len_selectors * sizeof(double2)),
                             stage_out(out, len_out * sizeof(W))};
    return handle_call(h->guard, h->fft->device, form, bufs, s, [&](void *const *ptr, hipStream_t st) -> int {
        const W *leaves = (const W *)ptr[0];
        // chunk after chunk; every stage of a chunk is queued before the next chunk starts
        for (u64 done = 0; done < batch; done += h->chunk) {
            const u64 cur = std::min<u64>(h->chunk, batch - done);
            const double2 *keys = (const double2 *)ptr[1] + done * p * h->key_len;
            // where the chunk's ciphertexts end: in the output, or in the owned buffer that stage C extracts from
            W *res = extract ? h->acc : (W *)ptr[2] + done * o * glwe;
            const W *src = shared ? leaves : leaves + ((done * o) << t) * glwe;
            for (u32 j = 0; j < t; ++j) {  // stage A: bit r + j halves the nodes of every (input, output)
                const u64 per_input = (u64)o << (t - 1 - j);
                W *dst = j + 1 == t ? res : h->tree->node[j & 1];
                const CmuxSources at{2 * glwe, per_input, (u64)p * h->key_len, j == 0 && shared ? (u32)per_input : 0u};
                PFHE_TRY(tfhe_cmux_launch<W>(h->tree.get(), src, src + glwe, keys + (h->r + j) * h->key_len, dst, cur * per_input,
                                             at, st));
                src = dst;
            }
            // stage B: in place on the tree's results, or from the table (its o ciphertexts shared, or the chunk's own); the
            // accumulators carry their global index, so the keys are the call's, not the chunk's
            const bool gather = t == 0 && shared;
            if (h->r > 0)
                PFHE_TRY(rotate_accs<W>(h, gather ? leaves : src, (const double2 *)ptr[1], res, done * o, cur * o, p,
                                        gather ? (u32)o : 0u, st));
            if (extract)  // stage C
                PFHE_TRY(launch_extract<W>(res, nullptr, (W *)ptr[2] + done * o * extract * (((u64)k << h->shape.log_n) + 1), k,
                                           h->shape.log_n, ExtractRule{(u32)extract, 0, (u32)extract, 0, 0, 0}, cur * o * extract,
                                           st));
        }
        return PFHE_OK;
    });
}

template <class H>
size_t lut_scratch(const H *h) {
    if (!h || !h->fft) return 0;
    const auto *tree = h->tree.get();
    return h->bufs.bytes() + (tree ? tree->bufs.bytes() + (tree->plan ? tree->plan->scratch.bytes() : 0) : 0);
}

}  // namespace

// The entry points of one word width.  P: pfhe_tfhe / pfhe_tfhe32; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_LUT_FAMILY(P, CW, W)                                                                                         \
    PFHE_ENTRY(P##_lut_create, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                           \
                size_t decompose_length, size_t tree_depth, size_t rot_bits, size_t log_stride, size_t outputs,           \
                size_t chunk, P##_lut_handle **out),                                                                      \
               lut_create<W>(fft, glwe_dimension, log_basis, decompose_length, tree_depth, rot_bits, log_stride, outputs, \
                             chunk, out))                                                                                 \
    PFHE_HANDLE_TRIO(P##_lut, P##_lut_handle, lut_scratch(h))                                                             \
    PFHE_ENTRY(P##_rotate_by_bits_dev, (P##_lut_handle *h, const CW *inp_dev, size_t len_inp, const double *keys_dev,     \
                size_t len_keys, size_t keys_per_input, size_t first_key, CW *out_dev, size_t len_out, void *stream),     \
               rotate_by_bits<W>(Form::kDevice, h, (const W *)inp_dev, len_inp, keys_dev, len_keys, keys_per_input,       \
                                 first_key, (W *)out_dev, len_out, (hipStream_t)stream))                                  \
    PFHE_ENTRY(P##_rotate_by_bits, (P##_lut_handle *h, const CW *inp, size_t len_inp, const double *keys,                 \
                size_t len_keys, size_t keys_per_input, size_t first_key, CW *out, size_t len_out),                       \
               rotate_by_bits<W>(Form::kHost, h, (const W *)inp, len_inp, keys, len_keys, keys_per_input, first_key,      \
                                 (W *)out, len_out, nullptr))                                                             \
    PFHE_ENTRY(P##_lut_eval_dev, (P##_lut_handle *h, const CW *table_dev, size_t len_table,                               \
                const double *selectors_dev, size_t len_selectors, size_t extract, CW *out_dev, size_t len_out,           \
                void *stream),                                                                                            \
               lut_eval<W>(Form::kDevice, h, (const W *)table_dev, len_table, selectors_dev, len_selectors, extract,      \
                           (W *)out_dev, len_out, (hipStream_t)stream))                                                   \
    PFHE_ENTRY(P##_lut_eval, (P##_lut_handle *h, const CW *table, size_t len_table, const double *selectors,              \
                size_t len_selectors, size_t extract, CW *out, size_t len_out),                                           \
               lut_eval<W>(Form::kHost, h, (const W *)table, len_table, selectors, len_selectors, extract, (W *)out,      \
                           len_out, nullptr))

extern "C" {

PFHE_LUT_FAMILY(pfhe_tfhe, uint64_t, u64)
PFHE_LUT_FAMILY(pfhe_tfhe32, uint32_t, u32)
#undef PFHE_LUT_FAMILY

}  // extern "C"
