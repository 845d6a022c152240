// pfhe_capi_internal.hpp — helpers shared by the extern "C" translation units.
#pragma once
#include <new>

#include "pfhe_common.hpp"
#include "pfhe_handles.hpp"

#define PFHE_GUARD_BEGIN try {
#define PFHE_GUARD_END                                   \
    }                                                    \
    catch (const std::bad_alloc &) {                     \
        ::pfhe::set_last_error("out of host memory");    \
        return PFHE_ERR_HIP;                             \
    }                                                    \
    catch (...) {                                        \
        ::pfhe::set_last_error("unexpected C++ exception"); \
        return PFHE_ERR_HIP;                             \
    }

// One entry point: guarded against exceptions, then the call.  A step with two forms passes its template Form::kDevice
// and the caller's stream, or Form::kHost and no stream.
//
// Every entry point that exists for both word widths is written once, in a family macro that its file defines just above
// its extern "C" block, expands once per width and #undef's after.  A family takes the name prefix (pfhe_tfhe /
// pfhe_tfhe32, ...), the word as pfhe.h spells it (CW: uint64_t / uint32_t) and as the library does (W: u64 / u32).
// uint64_t and u64 are two types here, so a family casts every word pointer to W; for u32 the cast is the identity.
#define PFHE_ENTRY(NAME, PARAMS, ...) \
    int NAME PARAMS {                 \
        PFHE_GUARD_BEGIN              \
        return __VA_ARGS__;           \
        PFHE_GUARD_END                \
    }

// What every handle with device scratch has: NAME_destroy, NAME_in_use and NAME_scratch_bytes of the handle type H.
// SCRATCH: the handle's scratch bytes, an expression over the non-null `h`.
#define PFHE_HANDLE_TRIO(NAME, H, SCRATCH)                                    \
    void NAME##_destroy(H *h) { delete h; }                                   \
    int NAME##_in_use(const H *h) { return h ? h->guard.in_use() : 0; }       \
    size_t NAME##_scratch_bytes(const H *h) { return h ? (SCRATCH) : 0; }

// The four table handles of pfhe.h: one base, four names.
struct pfhe_ntt : pfhe::TableHandle {};
struct pfhe_dcrt : pfhe::TableHandle {};
struct pfhe_ntt32 : pfhe::TableHandle {};
struct pfhe_dcrt32 : pfhe::TableHandle {};

namespace pfhe {
int capi_check_device(int device);
inline const TableSet *capi_table_of(const pfhe_dcrt *t) { return t->t.get(); }
inline const TableSet *capi_table32_of(const pfhe_dcrt32 *t) { return t->t.get(); }
// *_transform_pass_name: "u32:" in front of the longest name ntt_pass_name writes
constexpr size_t kPassNameCap = 4 + 96;
}  // namespace pfhe
