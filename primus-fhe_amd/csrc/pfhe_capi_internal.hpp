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
