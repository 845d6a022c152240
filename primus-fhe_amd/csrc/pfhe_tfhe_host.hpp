// pfhe_tfhe_host.hpp — the host layer under every torus entry point (pfhe_fft.hip, pfhe_bootstrap.hip, pfhe_keygen.hip):
// the constants they share, the launch of a torus kernel, and the staged run of a device form on host pointers.  Host only.
//
// A new torus entry point writes its own argument checks (in the order it wants them refused) and its launches through
// launch_flat / launch_groups / launch_grid; its host form repeats the checks that concern host pointers and hands the
// device form to staged_call.
#pragma once

#include "pfhe_fft_device.hpp"
#include "pfhe_staging.hpp"

namespace pfhe {

constexpr int kThreads = kFftThreads;  // every torus kernel runs workgroups of this many threads
constexpr u32 kMaxLogN = 14;           // the N/2-point transform of a polynomial lives in LDS
constexpr size_t kMaxGlweDimension = 64;
constexpr size_t kMaxGrouping = 4;

// ---------------- launches ----------------

// `grid` workgroups of kThreads threads with `lds` bytes of dynamic LDS, and the launch's own error
template <class K, class... Args>
int launch_grid(K kernel, dim3 grid, size_t lds, hipStream_t s, Args... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), lds, s, args...);
    PFHE_HIP(hipGetLastError());
    return PFHE_OK;
}

// `groups` workgroups in a row; more than a grid holds is refused
template <class K, class... Args>
int launch_groups(K kernel, u64 groups, size_t lds, hipStream_t s, Args... args) {
    if (groups > 0x7fffffffull) return PFHE_ERR_BAD_LENGTH;
    return launch_grid(kernel, dim3((u32)groups), lds, s, args...);
}

// one thread per element: `total` of them, which the kernel takes as its last argument
template <class K, class... Args>
int launch_flat(K kernel, u64 total, hipStream_t s, Args... args) {
    return launch_groups(kernel, (total + kThreads - 1) / kThreads, 0, s, args..., total);
}

// ---------------- host forms ----------------

// One buffer of a host form: `bytes` at `host` that the device form reads (in), writes (out) or both.  A buffer of no
// bytes is not staged: its device pointer stays null.
struct StageBuf {
    enum Dir { kIn, kOut, kInOut };
    void *host;
    size_t bytes;
    Dir dir;
};
inline StageBuf stage_in(const void *host, size_t bytes) { return {const_cast<void *>(host), bytes, StageBuf::kIn}; }
inline StageBuf stage_out(void *host, size_t bytes) { return {host, bytes, StageBuf::kOut}; }
inline StageBuf stage_inout(void *host, size_t bytes) { return {host, bytes, StageBuf::kInOut}; }

// The tail of every host form, arguments already checked: `device` made current, a pooled staging context, the ins and
// in/outs uploaded and the outs allocated in the order given, body(dev, stream) with dev[i] the device copy of bufs[i],
// the outs and in/outs downloaded, one wait.  PFHE_ERR_NO_DEVICE / PFHE_ERR_HIP when the device or the context cannot be
// had, otherwise the first status that is not PFHE_OK.
template <size_t N, class Body>
int staged_call(int device, const StageBuf (&bufs)[N], Body &&body) {
    DeviceGuard g(device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    HostStage st(device);
    if (!st.ok()) return PFHE_ERR_HIP;
    void *dev[N] = {};
    for (size_t i = 0; i < N; ++i) {
        if (!bufs[i].bytes) continue;
        PFHE_TRY(bufs[i].dir == StageBuf::kOut ? st.alloc(bufs[i].bytes, &dev[i]) : st.upload(bufs[i].host, bufs[i].bytes, &dev[i]));
    }
    PFHE_TRY(body(dev, st.stream()));
    for (size_t i = 0; i < N; ++i)
        if (bufs[i].bytes && bufs[i].dir != StageBuf::kIn) PFHE_TRY(st.download(bufs[i].host, dev[i], bufs[i].bytes));
    return st.finish();
}

// what the host forms of the rotations ask of their exponents (the device forms take them modulo 2N instead)
inline int require_exps_below_2n(const uint32_t *exps, size_t len, size_t n, const char *message) {
    for (size_t i = 0; i < len; ++i) {
        if (exps[i] >= 2 * n) {
            set_last_error(message);
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    return PFHE_OK;
}

// true when the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte
inline bool overlaps(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace pfhe
