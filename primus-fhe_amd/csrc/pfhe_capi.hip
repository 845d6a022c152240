// pfhe_capi.hip — extern "C" boundary (include/pfhe.h).  Validates arguments, owns handles,
// never throws.  There is deliberately no CPU fallback: without a HIP device every create()
// fails with PFHE_ERR_NO_DEVICE.
//
// Here: the process-wide plumbing (last error, DeviceGuard, device memory), the host layer of the four table handles —
// one template over the word type per operation — and their entry points.  Table construction: pfhe_tables.cpp; the
// host-slice transform: pfhe_staging.cpp; the u32 streaming kernels and their launchers: pfhe_u32.hip.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "pfhe_capi_internal.hpp"
#include "pfhe_common.hpp"
#include "pfhe_handles.hpp"
#include "pfhe_ntt_device.hpp"
#include "pfhe_pointwise.hpp"
#include "pfhe_staging.hpp"

namespace pfhe {

static thread_local std::string g_last_error;

void set_last_error(const std::string &msg) { g_last_error = msg; }

int hip_fail(hipError_t e, const char *what, const char *file, int line) {
    char buf[512];
    std::snprintf(buf, sizeof buf, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    g_last_error = buf;
    (void)hipGetLastError();  // clear the sticky error
    return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? PFHE_ERR_NO_DEVICE : PFHE_ERR_HIP;
}

static thread_local int g_guard_depth = 0;

DeviceGuard::DeviceGuard(int device) {
    // hipGetLastError() is per host thread and sticky: an error the CALLER's own earlier HIP call left behind (a refused
    // hipHostRegister, say) would otherwise be reported by the first launch check of this entry point as if a kernel of
    // this library had failed (found by tools/hazard_suite_probe.sh, round 5).  Every entry point starts from a clean slate —
    // the OUTERMOST guard of a call only: entry points call one another (host-pointer forms call the device ones), and a
    // nested guard must not swallow the error of a launch this library queued a moment earlier.  (The caller's stale code
    // is consumed; include/pfhe.h says so: check your own HIP calls' return values.)
    if (g_guard_depth++ == 0) (void)hipGetLastError();
    if (hipGetDevice(&prev) != hipSuccess) {
        prev = -1;
        (void)hipGetLastError();
    }
    ok = hipSetDevice(device) == hipSuccess;
    if (!ok) (void)hipGetLastError();
}
DeviceGuard::~DeviceGuard() {
    --g_guard_depth;
    if (prev >= 0) (void)hipSetDevice(prev);
}

int capi_check_device(int device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        set_last_error("no HIP device available (libpfhe_hip has no CPU fallback)");
        return PFHE_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= count) {
        set_last_error("device index out of range");
        return PFHE_ERR_NO_DEVICE;
    }
    return PFHE_OK;
}

int check_len(const TableSet &t, size_t len, u64 &units) {
    const size_t unit = t.n * t.L;
    if (len % unit != 0) {
        set_last_error("slice length is not a multiple of the polynomial length");
        return PFHE_ERR_BAD_LENGTH;
    }
    units = len / unit;
    return PFHE_OK;
}

template <class W>
int transform_dev(const TableSet &t, W *data, size_t len, bool inverse, bool lazy, hipStream_t s) {
    if (!data && len) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(data);
    u64 units = 0;
    PFHE_TRY(check_len(t, len, units));
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return launch_transform(t, data, units * t.L, inverse, lazy, s);
}

template <class W>
int pointwise(const TableSet &t, int mode, W *acc, const W *a, size_t len_a, const W *b, size_t len_b, hipStream_t s) {
    if ((!acc || !b || (mode == 1 && !a)) && len_a) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(acc);
    PFHE_REQUIRE_ALIGNED(a);
    PFHE_REQUIRE_ALIGNED(b);
    u64 units = 0;
    PFHE_TRY(check_len(t, len_a, units));
    if (len_b != len_a && len_b != t.n * t.L) {
        set_last_error("multiplicand must have the same length or exactly one polynomial");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_a == 0) return PFHE_OK;
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return launch_pointwise(t, mode, acc, a, b, len_a, len_b, s);
}

// out = a*b (+ c): NttPolynomial::mul_to / mul_add_to (primus_poly/src/ntt/mul.rs:100-107, ntt/mod.rs:169-187)
int pointwise_to(const TableSet &t, u64 *out, const u64 *a, size_t len_a, const u64 *b, size_t len_b, const u64 *c,
                 bool has_c, hipStream_t s) {
    if ((!out || !a || !b || (has_c && !c)) && len_a) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(out);
    PFHE_REQUIRE_ALIGNED(a);
    PFHE_REQUIRE_ALIGNED(b);
    PFHE_REQUIRE_ALIGNED(c);
    u64 units = 0;
    PFHE_TRY(check_len(t, len_a, units));
    if (len_b != len_a && len_b != t.n * t.L) {
        set_last_error("multiplicand must have the same length or exactly one polynomial");
        return PFHE_ERR_BAD_LENGTH;
    }
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return pointwise_dev(out, a, b, has_c ? c : nullptr, t.primes_dev, t.L, t.log_n, len_a, len_b, s, 0, t.pm);
}

template <class W>
int monomial(const TableSet &t, W coeff, size_t degree, W *values, size_t len, bool host, hipStream_t s, bool minus_one) {
    if (!values) return PFHE_ERR_BAD_ARGUMENT;
    if (len != t.n * t.L) {
        set_last_error("monomial output must be exactly one polynomial");
        return PFHE_ERR_BAD_LENGTH;
    }
    // the per-limb scalars travel by value as kernel arguments (no staging buffer: the device form is capturable), at most
    // kMaxMonomialLimbs of them per launch; wider bases take one launch per group of limbs
    std::vector<MonomialScalars> groups((t.L + kMaxMonomialLimbs - 1) / kMaxMonomialLimbs);
    for (u32 i = 0; i < t.L; ++i) {
        const W q = (W)t.primes[i].q;
        const W ci = minus_one ? q - 1 : coeff;
        if (ci >= q) {
            set_last_error("monomial coefficient must be reduced modulo every modulus");
            return PFHE_ERR_BAD_ARGUMENT;
        }
        MonomialScalars &sc = groups[i / kMaxMonomialLimbs];
        sc.value[i % kMaxMonomialLimbs] = ci;
        sc.quotient[i % kMaxMonomialLimbs] = monomial_quotient(ci, q);
    }
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    const u64 deg = (u64)degree & (2 * (u64)t.n - 1);
    const auto run = [&](W *out, hipStream_t st) -> int {
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            const u32 l0 = (u32)gi * kMaxMonomialLimbs, lg = std::min<u32>(kMaxMonomialLimbs, t.L - l0);
            PFHE_TRY(launch_monomial(out + (size_t)l0 * t.n, t.primes_dev + l0, lg, t.log_n, deg, groups[gi], st));
        }
        return PFHE_OK;
    };
    if (!host)  // device output: launches on the caller's stream, nothing else (capturable)
        return run(values, s);
    // host output: the caller's stream is not involved (pooled staging context, no allocation in steady state)
    const StageBuf bufs[] = {stage_out(values, len * sizeof(W))};
    return staged_call(t.device, bufs, [&](void *const *d, hipStream_t st) { return run(static_cast<W *>(d[0]), st); });
}

#define PFHE_TABLE_HOST_LAYER(W)                                                                                          \
    template int transform_dev<W>(const TableSet &, W *, size_t, bool, bool, hipStream_t);                                \
    template int pointwise<W>(const TableSet &, int, W *, const W *, size_t, const W *, size_t, hipStream_t);             \
    template int monomial<W>(const TableSet &, W, size_t, W *, size_t, bool, hipStream_t, bool);
PFHE_TABLE_HOST_LAYER(u64)
PFHE_TABLE_HOST_LAYER(u32)
#undef PFHE_TABLE_HOST_LAYER

// what the four create() entry points share: `make` is make_table_set or make_table_set32
template <class H, class W, class Make>
int create_table(Make make, u32 log_n, const W *moduli, size_t count, int device, H **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    std::unique_ptr<TableSet> t;
    PFHE_TRY(make(log_n, moduli, count, device, t));
    *out = new H{{std::move(t)}};
    return PFHE_OK;
}

}  // namespace pfhe

using namespace pfhe;

extern "C" {

const char *pfhe_status_string(int status) {
    switch (status) {
        case PFHE_OK: return "ok";
        case PFHE_ERR_NO_PRIMITIVE_ROOT: return "there is no primitive root with this degree and modulus";
        case PFHE_ERR_DEGREE_CONVERSION: return "out of range integral type conversion attempted";
        case PFHE_ERR_DEGREE_TOO_LARGE: return "degree should be less than modulus";
        case PFHE_ERR_NTT_TABLE: return "failed to generate the desired ntt table";
        case PFHE_ERR_MODULUS_TOO_LARGE: return "modulus is too large for this NTT table (max 62-bit supported)";
        case PFHE_ERR_EMPTY_BASE: return "RNS base is empty";
        case PFHE_ERR_COPRIME: return "RNS moduli are not pairwise coprime";
        case PFHE_ERR_UNREPRESENTABLE_MODULUS: return "RNS modulus is not representable";
        case PFHE_ERR_BAD_LENGTH: return "slice length does not match the table";
        case PFHE_ERR_BAD_ARGUMENT: return "bad argument";
        case PFHE_ERR_NO_DEVICE: return "no usable HIP device";
        case PFHE_ERR_HIP: return "HIP runtime error";
        case PFHE_ERR_UNSUPPORTED: return "unsupported parameter";
        case PFHE_ERR_NO_INVERSE: return "element has no inverse";
        case PFHE_ERR_BUSY: return "external-product plan is held by another thread";
    }
    return "unknown status";
}

const char *pfhe_last_error(void) { return g_last_error.c_str(); }
const char *pfhe_version(void) { return "libpfhe_hip 0.1.0 gfx950"; }

int pfhe_device_count(int *count) {
    if (!count) return PFHE_ERR_BAD_ARGUMENT;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) {
        (void)hipGetLastError();
        c = 0;
    }
    *count = c;
    return PFHE_OK;
}

uint64_t pfhe_debug_alloc_count(void) { return alloc_event_count(); }
uint64_t pfhe_debug_stage_path_count(int which) { return stage_path_count(which); }
int pfhe_staging_release(int device) { return staging_release(device); }

int pfhe_device_malloc(int device, size_t bytes, void **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    PFHE_TRY(capi_check_device(device));
    DeviceGuard g(device);
    if (bytes == 0) return PFHE_OK;
    PFHE_HIP(counted_malloc(out, bytes));
    return PFHE_OK;
}

int pfhe_device_free(int device, void *ptr) {
    if (!ptr) return PFHE_OK;
    PFHE_TRY(capi_check_device(device));
    DeviceGuard g(device);
    PFHE_HIP(counted_free(ptr));
    return PFHE_OK;
}

int pfhe_memcpy_h2d(int device, void *dst, const void *src, size_t bytes, void *stream) {
    if (bytes == 0) return PFHE_OK;
    if (!dst || !src) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_TRY(capi_check_device(device));
    DeviceGuard g(device);
    PFHE_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    PFHE_HIP(hipStreamSynchronize((hipStream_t)stream));
    return PFHE_OK;
}

int pfhe_memcpy_d2h(int device, void *dst, const void *src, size_t bytes, void *stream) {
    if (bytes == 0) return PFHE_OK;
    if (!dst || !src) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_TRY(capi_check_device(device));
    DeviceGuard g(device);
    PFHE_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    PFHE_HIP(hipStreamSynchronize((hipStream_t)stream));
    return PFHE_OK;
}

int pfhe_memcpy_d2d(int device, void *dst, const void *src, size_t bytes, void *stream) {
    if (bytes == 0) return PFHE_OK;
    if (!dst || !src) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_TRY(capi_check_device(device));
    DeviceGuard g(device);
    PFHE_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PFHE_OK;
}

int pfhe_memset_dev(int device, void *dst, int byte, size_t bytes, void *stream) {
    if (bytes == 0) return PFHE_OK;
    if (!dst) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_TRY(capi_check_device(device));
    DeviceGuard g(device);
    PFHE_HIP(hipMemsetAsync(dst, byte, bytes, (hipStream_t)stream));
    return PFHE_OK;
}

int pfhe_stream_synchronize(int device, void *stream) {
    PFHE_TRY(capi_check_device(device));
    DeviceGuard g(device);
    PFHE_HIP(hipStreamSynchronize((hipStream_t)stream));
    return PFHE_OK;
}

int pfhe_fill_uniform_dev(int device, uint64_t *dst, size_t len, const uint64_t *moduli, size_t moduli_count,
                          size_t poly_len, uint64_t seed, void *stream) {
    PFHE_GUARD_BEGIN
    if (len == 0) return PFHE_OK;
    if (!dst || !moduli || moduli_count == 0 || poly_len == 0) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_TRY(capi_check_device(device));
    DeviceGuard g(device);
    // not a staged_call: the list is uploaded and waited for, then the kernel runs on the caller's stream
    HostStage st(device);  // the modulus list travels through a pooled staging context (no allocation per call)
    if (!st.ok()) return PFHE_ERR_HIP;
    void *md = nullptr;
    PFHE_TRY(st.upload(moduli, moduli_count * sizeof(u64), &md));
    PFHE_TRY(st.finish());
    PFHE_TRY(fill_uniform_dev((u64 *)dst, len, (const u64 *)md, moduli_count, poly_len, seed, (hipStream_t)stream));
    PFHE_HIP(hipStreamSynchronize((hipStream_t)stream));  // the list must outlive the kernel
    return PFHE_OK;
    PFHE_GUARD_END
}

/* ------------- the four tables: U64NttTable, U64DcrtTable, U32NttTable, U32DcrtTable ------------- */

int pfhe_ntt_create(uint32_t log_n, uint64_t modulus, int device, pfhe_ntt **out) {
    PFHE_GUARD_BEGIN
    const u64 q = modulus;
    return create_table(make_table_set, log_n, &q, 1, device, out);
    PFHE_GUARD_END
}
int pfhe_dcrt_create(uint32_t log_n, const uint64_t *moduli, size_t moduli_count, int device, pfhe_dcrt **out) {
    PFHE_GUARD_BEGIN
    if (!out || (!moduli && moduli_count)) return PFHE_ERR_BAD_ARGUMENT;
    return create_table(make_table_set, log_n, (const u64 *)moduli, moduli_count, device, out);
    PFHE_GUARD_END
}
int pfhe_ntt32_create(uint32_t log_n, uint32_t modulus, int device, pfhe_ntt32 **out) {
    PFHE_GUARD_BEGIN
    const u32 q = modulus;
    return create_table(make_table_set32, log_n, &q, 1, device, out);
    PFHE_GUARD_END
}
int pfhe_dcrt32_create(uint32_t log_n, const uint32_t *moduli, size_t moduli_count, int device, pfhe_dcrt32 **out) {
    PFHE_GUARD_BEGIN
    return create_table(make_table_set32, log_n, moduli, moduli_count, device, out);  // (refuses a null list itself)
    PFHE_GUARD_END
}

// An entry point of a table: PFHE_ENTRY that refuses a null `table` before the call.
#define PFHE_ENTRY_TABLE(NAME, PARAMS, ...) PFHE_ENTRY(NAME, PARAMS, table ? (__VA_ARGS__) : PFHE_ERR_BAD_ARGUMENT)

// What the four handles share.  H: the handle type, whose name is also the symbol prefix; W / CW: the word type as the
// host layer and as pfhe.h spell it.
#define PFHE_TABLE_FAMILY(H, W, CW)                                                                                      \
    void H##_destroy(H *table) { delete table; }                                                                         \
    size_t H##_poly_length(const H *t) { return t ? t->t->n : 0; }                                                       \
    int H##_device(const H *t) { return t ? t->t->device : -1; }                                                         \
    PFHE_ENTRY_TABLE(H##_transform_slice, (const H *table, CW *p, size_t len),                                           \
                     transform_host(*table->t, (W *)p, len, false, false))                                               \
    PFHE_ENTRY_TABLE(H##_inverse_transform_slice, (const H *table, CW *p, size_t len),                                   \
                     transform_host(*table->t, (W *)p, len, true, false))                                                \
    PFHE_ENTRY_TABLE(H##_lazy_transform_slice, (const H *table, CW *p, size_t len),                                      \
                     transform_host(*table->t, (W *)p, len, false, true))                                                \
    PFHE_ENTRY_TABLE(H##_lazy_inverse_transform_slice, (const H *table, CW *p, size_t len),                              \
                     transform_host(*table->t, (W *)p, len, true, true))                                                 \
    PFHE_ENTRY_TABLE(H##_transform_monomial, (const H *table, CW coeff, size_t degree, CW *values, size_t len),          \
                     monomial<W>(*table->t, coeff, degree, (W *)values, len, true, nullptr))                             \
    PFHE_ENTRY_TABLE(H##_transform_coeff_one_monomial, (const H *table, size_t degree, CW *values, size_t len),          \
                     monomial<W>(*table->t, 1, degree, (W *)values, len, true, nullptr))                                 \
    PFHE_ENTRY_TABLE(H##_transform_coeff_minus_one_monomial, (const H *table, size_t degree, CW *values, size_t len),    \
                     monomial<W>(*table->t, 0, degree, (W *)values, len, true, nullptr, /*minus_one=*/true))             \
    PFHE_ENTRY_TABLE(H##_transform_dev, (const H *table, CW *poly_dev, size_t len, int lazy, void *stream),              \
                     transform_dev(*table->t, (W *)poly_dev, len, false, lazy != 0, (hipStream_t)stream))                \
    PFHE_ENTRY_TABLE(H##_inverse_transform_dev, (const H *table, CW *values_dev, size_t len, int lazy, void *stream),    \
                     transform_dev(*table->t, (W *)values_dev, len, true, lazy != 0, (hipStream_t)stream))               \
    PFHE_ENTRY_TABLE(H##_mul_assign_dev,                                                                                 \
                     (const H *table, CW *a_dev, size_t len_a, const CW *b_dev, size_t len_b, void *stream),             \
                     pointwise<W>(*table->t, 0, (W *)a_dev, nullptr, len_a, (const W *)b_dev, len_b, (hipStream_t)stream)) \
    PFHE_ENTRY_TABLE(H##_add_mul_assign_dev,                                                                             \
                     (const H *table, CW *acc_dev, const CW *a_dev, size_t len_a, const CW *b_dev, size_t len_b,         \
                      void *stream),                                                                                     \
                     pointwise<W>(*table->t, 1, (W *)acc_dev, (const W *)a_dev, len_a, (const W *)b_dev, len_b,          \
                                  (hipStream_t)stream))

// the constants of the one prime of an NttTable (table.rs:127-161) / of limb i of a DcrtTable
#define PFHE_NTT_GETTERS(H, CW)                                                     \
    uint32_t H##_log_n(const H *t) { return t ? t->t->log_n : 0; }                  \
    CW H##_modulus(const H *t) { return t ? (CW)t->t->primes[0].q : 0; }            \
    CW H##_root(const H *t) { return t ? (CW)t->t->roots[0] : 0; }                  \
    CW H##_inv_root(const H *t) { return t ? (CW)t->t->inv_roots[0] : 0; }          \
    CW H##_inv_n(const H *t) { return t ? (CW)t->t->primes[0].inv_n : 0; }
#define PFHE_DCRT_GETTERS(H, CW)                                                                      \
    size_t H##_moduli_count(const H *t) { return t ? t->t->L : 0; }                                   \
    size_t H##_crt_poly_length(const H *t) { return t ? t->t->n * t->t->L : 0; }                      \
    CW H##_modulus(const H *t, size_t i) { return (t && i < t->t->L) ? (CW)t->t->primes[i].q : 0; }   \
    CW H##_root(const H *t, size_t i) { return (t && i < t->t->L) ? (CW)t->t->roots[i] : 0; }

// out = a*b (+ c): the u64 tables only
#define PFHE_TABLE_MUL_TO(H)                                                                                              \
    PFHE_ENTRY_TABLE(H##_mul_to_dev,                                                                                      \
                     (const H *table, const uint64_t *a_dev, size_t len_a, const uint64_t *b_dev, size_t len_b,           \
                      uint64_t *out_dev, void *stream),                                                                   \
                     pointwise_to(*table->t, (u64 *)out_dev, (const u64 *)a_dev, len_a, (const u64 *)b_dev, len_b,        \
                                  nullptr, false, (hipStream_t)stream))                                                   \
    PFHE_ENTRY_TABLE(H##_mul_add_to_dev,                                                                                  \
                     (const H *table, const uint64_t *a_dev, size_t len_a, const uint64_t *b_dev, size_t len_b,           \
                      const uint64_t *c_dev, uint64_t *out_dev, void *stream),                                            \
                     pointwise_to(*table->t, (u64 *)out_dev, (const u64 *)a_dev, len_a, (const u64 *)b_dev, len_b,        \
                                  (const u64 *)c_dev, true, (hipStream_t)stream))

PFHE_TABLE_FAMILY(pfhe_ntt, u64, uint64_t)
PFHE_TABLE_FAMILY(pfhe_dcrt, u64, uint64_t)
PFHE_TABLE_FAMILY(pfhe_ntt32, u32, uint32_t)
PFHE_TABLE_FAMILY(pfhe_dcrt32, u32, uint32_t)
PFHE_NTT_GETTERS(pfhe_ntt, uint64_t)
PFHE_NTT_GETTERS(pfhe_ntt32, uint32_t)
PFHE_DCRT_GETTERS(pfhe_dcrt, uint64_t)
PFHE_DCRT_GETTERS(pfhe_dcrt32, uint32_t)
PFHE_TABLE_MUL_TO(pfhe_ntt)
PFHE_TABLE_MUL_TO(pfhe_dcrt)
#undef PFHE_TABLE_FAMILY
#undef PFHE_NTT_GETTERS
#undef PFHE_DCRT_GETTERS
#undef PFHE_TABLE_MUL_TO

uint64_t pfhe_dcrt_inv_n(const pfhe_dcrt *t, size_t i) { return (t && i < t->t->L) ? t->t->primes[i].inv_n : 0; }

/* ---------------------------- entry points one table has ---------------------------- */

PFHE_ENTRY_TABLE(pfhe_ntt_transform_monomial_dev,
                 (const pfhe_ntt *table, uint64_t coeff, size_t degree, uint64_t *values_dev, size_t len, void *stream),
                 monomial<u64>(*table->t, coeff, degree, (u64 *)values_dev, len, false, (hipStream_t)stream))
PFHE_ENTRY_TABLE(pfhe_ntt32_transform_monomial_dev,
                 (const pfhe_ntt32 *table, uint32_t coeff, size_t degree, uint32_t *values_dev, size_t len, void *stream),
                 monomial<u32>(*table->t, coeff, degree, values_dev, len, false, (hipStream_t)stream))

int pfhe_dcrt_transform_monomial_dev(const pfhe_dcrt *table, uint64_t coeff, size_t degree, uint64_t *values_dev,
                                     size_t len, int minus_one, void *stream) {
    PFHE_GUARD_BEGIN
    if (!table) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(values_dev);
    return monomial<u64>(*table->t, minus_one ? 0 : coeff, degree, (u64 *)values_dev, len, false, (hipStream_t)stream,
                         minus_one != 0);
    PFHE_GUARD_END
}
#undef PFHE_ENTRY_TABLE

static int butterfly_api(const pfhe_dcrt *table, bool factor, uint64_t *a_dev, const uint64_t *rhs_dev, size_t len,
                         const uint64_t *w_dev, size_t len_w, uint64_t *result_dev, void *stream) {
    if (!table) return PFHE_ERR_BAD_ARGUMENT;
    const TableSet &t = *table->t;
    const size_t unit = t.n * t.L;
    if (len % unit != 0 || (len_w != unit * (factor ? 2 : 1) && len_w != len * (factor ? 2 : 1))) {
        set_last_error("butterfly: slices must be multiples of L*N words; the multiplicand is one polynomial "
                       "(shared) or matches the batch (ShoupFactor slices count two words per coefficient)");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len == 0) return PFHE_OK;
    if (!a_dev || !rhs_dev || !w_dev || !result_dev) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(a_dev);
    PFHE_REQUIRE_ALIGNED(rhs_dev);
    PFHE_REQUIRE_ALIGNED(w_dev);
    PFHE_REQUIRE_ALIGNED(result_dev);
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return butterfly_dev(factor, (u64 *)a_dev, (const u64 *)rhs_dev, (const u64 *)w_dev, (u64 *)result_dev, t.primes_dev,
                         t.L, t.log_n, len, factor ? len_w / 2 : len_w, (hipStream_t)stream, t.pm);
}

int pfhe_dcrt_butterfly_mul_dcrt_polynomial_to_dev(const pfhe_dcrt *table, uint64_t *a_dev, const uint64_t *rhs_dev,
                                                   size_t len, const uint64_t *dcrt_poly_dev, size_t len_w,
                                                   uint64_t *result_dev, void *stream) {
    PFHE_GUARD_BEGIN
    return butterfly_api(table, false, a_dev, rhs_dev, len, dcrt_poly_dev, len_w, result_dev, stream);
    PFHE_GUARD_END
}

int pfhe_dcrt_butterfly_mul_factor_to_dev(const pfhe_dcrt *table, uint64_t *a_dev, const uint64_t *rhs_dev, size_t len,
                                          const uint64_t *factor_poly_dev, size_t len_w, uint64_t *result_dev,
                                          void *stream) {
    PFHE_GUARD_BEGIN
    return butterfly_api(table, true, a_dev, rhs_dev, len, factor_poly_dev, len_w, result_dev, stream);
    PFHE_GUARD_END
}

int pfhe_dcrt_add_dcrt_glwe_mul_dcrt_polynomial_assign_dev(const pfhe_dcrt *table, uint64_t *acc_dev,
                                                           const uint64_t *dcrt_glwe_dev, size_t len,
                                                           const uint64_t *dcrt_poly_dev, size_t len_poly,
                                                           size_t glwe_polys, void *stream) {
    PFHE_GUARD_BEGIN
    if (!table || glwe_polys == 0 || ((!acc_dev || !dcrt_glwe_dev || !dcrt_poly_dev) && len)) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(acc_dev);
    PFHE_REQUIRE_ALIGNED(dcrt_glwe_dev);
    PFHE_REQUIRE_ALIGNED(dcrt_poly_dev);
    const TableSet &t = *table->t;
    const size_t unit = t.n * t.L;
    if (len % (unit * glwe_polys) != 0 || len_poly != len / glwe_polys) {
        set_last_error("expected batch*(k+1) polynomials in acc / glwe and batch polynomials in dcrt_poly");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len == 0) return PFHE_OK;
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return pointwise_dev((u64 *)acc_dev, (const u64 *)dcrt_glwe_dev, (const u64 *)dcrt_poly_dev, (const u64 *)acc_dev,
                         t.primes_dev, t.L, t.log_n, len, len_poly, (hipStream_t)stream, (u64)unit * glwe_polys, t.pm);
    PFHE_GUARD_END
}

int pfhe_dcrt_glwe_mul_dcrt_polynomial_to_dev(const pfhe_dcrt *table, const uint64_t *dcrt_glwe_dev, size_t len,
                                              const uint64_t *dcrt_poly_dev, size_t len_poly, size_t glwe_polys,
                                              uint64_t *result_dev, void *stream) {
    PFHE_GUARD_BEGIN
    if (!table || glwe_polys == 0 || ((!result_dev || !dcrt_glwe_dev || !dcrt_poly_dev) && len)) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(result_dev);
    PFHE_REQUIRE_ALIGNED(dcrt_glwe_dev);
    PFHE_REQUIRE_ALIGNED(dcrt_poly_dev);
    const TableSet &t = *table->t;
    const size_t unit = t.n * t.L;
    if (len % (unit * glwe_polys) != 0 || len_poly != len / glwe_polys) {
        set_last_error("expected batch*(k+1) polynomials in the glwe / result and batch polynomials in dcrt_poly");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len == 0) return PFHE_OK;
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return pointwise_dev((u64 *)result_dev, (const u64 *)dcrt_glwe_dev, (const u64 *)dcrt_poly_dev, nullptr, t.primes_dev,
                         t.L, t.log_n, len, len_poly, (hipStream_t)stream, (u64)unit * glwe_polys, t.pm);
    PFHE_GUARD_END
}

int pfhe_dcrt_transform_num_passes(const pfhe_dcrt *table) {
    return table ? ntt_num_passes(table->t->log_n, table->t->ntt_arith) : 0;
}

const char *pfhe_dcrt_transform_pass_name(const pfhe_dcrt *table, int inverse, int index) {
    static thread_local char buf[kPassNameCap];
    buf[0] = 0;
    if (table) ntt_pass_name(table->t->log_n, inverse != 0, index, buf, sizeof buf, table->t->ntt_arith);
    return buf;
}

int pfhe_dcrt_transform_form(const pfhe_dcrt *table, size_t len, int inverse, char *name, size_t cap, int *launches) {
    if (!table || !name || cap == 0 || !launches) return PFHE_ERR_BAD_ARGUMENT;
    const TableSet &t = *table->t;
    if (len % (t.n * t.L) != 0) return PFHE_ERR_BAD_LENGTH;
    *launches = ntt_transform_form(t.L, t.log_n, t.ntt_arith, len / t.n, inverse != 0, t.tune, name, cap);
    return PFHE_OK;
}

int pfhe_dcrt_transform_pass_dev(const pfhe_dcrt *table, uint64_t *poly_dev, size_t len, int inverse, int index,
                                 int lazy, void *stream) {
    PFHE_GUARD_BEGIN
    if (!table || (!poly_dev && len)) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(poly_dev);
    const TableSet &t = *table->t;
    if (len % (t.n * t.L) != 0) return PFHE_ERR_BAD_LENGTH;
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return ntt_pass_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, (u64 *)poly_dev, len / t.n, inverse != 0, index,
                        lazy != 0, (hipStream_t)stream);
    PFHE_GUARD_END
}

int pfhe_dcrt_mul_dcrt_polynomial_dev(const pfhe_dcrt *table, uint64_t *crt_poly_dev, size_t len,
                                      const uint64_t *dcrt_poly_dev, size_t len_b, void *stream) {
    PFHE_GUARD_BEGIN
    if (!table) return PFHE_ERR_BAD_ARGUMENT;
    const TableSet &t = *table->t;
    // every argument is checked BEFORE the forward transform is enqueued: a call that fails leaves the caller's
    // polynomial in coefficient form
    if ((!crt_poly_dev || !dcrt_poly_dev) && len) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(crt_poly_dev);
    PFHE_REQUIRE_ALIGNED(dcrt_poly_dev);
    if (len % (t.n * t.L) != 0) {
        set_last_error("slice length is not a multiple of the polynomial length");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_b != len && len_b != t.n * t.L) {
        set_last_error("multiplicand must have the same length or exactly one polynomial");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len != 0) {
        // forward block pass -> product -> inverse block pass in one kernel, between the strided passes
        DeviceGuard g(t.device);
        if (!g.ok) return PFHE_ERR_NO_DEVICE;
        const int rc = ntt_polymul_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, (u64 *)crt_poly_dev, len / t.n,
                                       (const u64 *)dcrt_poly_dev, len_b / t.n, (hipStream_t)stream, t.tune);
        if (rc != PFHE_ERR_UNSUPPORTED) return rc;
    }
    PFHE_TRY(transform_dev(t, (u64 *)crt_poly_dev, len, false, false, (hipStream_t)stream));
    if (t.log_n >= 4 && len != 0) {
        // shapes the fused kernel does not cover: the pointwise product rides on the loads of the inverse transform's first pass
        DeviceGuard g(t.device);
        if (!g.ok) return PFHE_ERR_NO_DEVICE;
        return ntt_inverse_mul_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, (u64 *)crt_poly_dev, len / t.n,
                                   (const u64 *)dcrt_poly_dev, len_b / t.n, (hipStream_t)stream, t.tune);
    }
    PFHE_TRY(pointwise<u64>(t, 0, (u64 *)crt_poly_dev, nullptr, len, (const u64 *)dcrt_poly_dev, len_b,
                       (hipStream_t)stream));
    return transform_dev(t, (u64 *)crt_poly_dev, len, true, false, (hipStream_t)stream);
    PFHE_GUARD_END
}

}  // extern "C"
