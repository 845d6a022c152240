// pfhe_tfhe_host.hpp — the host layer under every torus entry point (pfhe_fft.hip, pfhe_bootstrap.hip, pfhe_keygen.hip,
// pfhe_pack.hip): the constants and range tests they share, the launch of a torus kernel, the staged run of a launch on
// host pointers, and the one tail of the stateless steps.  Host only.
//
// A handle call (product, rotations, bootstrap) writes its checks in its device form; its host form re-enters that under
// the handle's lease through staged_call.  A stateless step is ONE function template for both of its forms:
//    1. it takes the Form (the extern "C" wrappers pass Form::kHost or Form::kDevice; a device-only step has none);
//    2. it runs its own argument checks in the order it wants them refused (require_lwe_dimension / _glwe_dimension
//       for the ranges), every one of them on values, none on a pointer;
//    3. it returns PFHE_OK for an empty batch;
//    4. it lists its buffers as StageBufs: stage_in / stage_out / stage_inout say which of them the kernels write;
//    5. it hands them to stateless_call with the device (the table's, or the caller's index), the message of its overlap
//       refusal, the stream and a callback (pointers, stream) that launches through launch_flat / _groups / _grid;
//    6. a check that has to come after the pointer tests (capi_check_device of a caller's index, the size of a launch) goes
//       in as the gate.
// stateless_call then refuses, in this order: a null buffer; in the device form a written buffer that shares a byte with
// any other buffer of the call (inputs may overlap each other, and the host form refuses no overlap: it stages); what
// the gate refuses; a device that cannot be made current.  Nothing is kept between calls.
#pragma once

#include <algorithm>

#include "pfhe_fft_device.hpp"
#include "pfhe_staging.hpp"

namespace pfhe {

constexpr int kThreads = kFftThreads;  // every torus kernel runs workgroups of this many threads
constexpr u32 kMaxLogN = 14;           // the N/2-point transform of a polynomial lives in LDS
constexpr size_t kMaxGlweDimension = 64;
constexpr size_t kMaxGrouping = 4;

// the range tests of the two dimensions, refused with the step's own message
inline int require_lwe_dimension(size_t dimension, const char *message) {
    if (dimension >= 1 && dimension < 0x7fffffffull) return PFHE_OK;  // 1..2^31-2
    set_last_error(message);
    return PFHE_ERR_BAD_ARGUMENT;
}
inline int require_glwe_dimension(size_t k, const char *message) {
    if (k >= 1 && k <= kMaxGlweDimension) return PFHE_OK;
    set_last_error(message);
    return PFHE_ERR_BAD_ARGUMENT;
}

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

// a 2-D launch whose y count exceeds what grid.y holds, in slices: launch(first, count) with count <= 65535
template <class Launch>
int launch_y_slices(u64 count, Launch &&launch) {
    for (u64 first = 0; first < count;) {
        const u32 cur = (u32)std::min<u64>(count - first, 65535);
        PFHE_TRY(launch(first, cur));
        first += cur;
    }
    return PFHE_OK;
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

// ---------------- the stateless steps ----------------

enum class Form { kHost, kDevice };

template <size_t N>
int refuse_null(const StageBuf (&bufs)[N]) {
    for (const StageBuf &b : bufs)
        if (b.bytes && !b.host) return PFHE_ERR_BAD_ARGUMENT;
    return PFHE_OK;
}

struct NoGate {
    int operator()() const { return PFHE_OK; }
};

// The tail of every stateless step, values already checked and the batch not empty (the recipe is at the top of this file).
// Device form: launch(pointers, s) on the caller's pointers and stream, with pointers[i] = bufs[i].host.  Host form:
// staged_call.  overlap_message null: the step refuses no overlap.
template <size_t N, class Launch, class Gate = NoGate>
int stateless_call(int device, Form form, const StageBuf (&bufs)[N], const char *overlap_message, hipStream_t s,
                   Launch &&launch, Gate &&gate = Gate{}) {
    PFHE_TRY(refuse_null(bufs));
    if (form == Form::kHost) {
        PFHE_TRY(gate());
        return staged_call(device, bufs, launch);
    }
    void *dev[N];
    for (size_t i = 0; i < N; ++i) {
        dev[i] = bufs[i].host;
        for (size_t j = 0; overlap_message && bufs[i].dir != StageBuf::kIn && j < N; ++j) {
            if (j != i && bufs[i].bytes && bufs[j].bytes && overlaps(dev[i], bufs[i].bytes, bufs[j].host, bufs[j].bytes)) {
                set_last_error(overlap_message);
                return PFHE_ERR_BAD_ARGUMENT;
            }
        }
    }
    PFHE_TRY(gate());
    DeviceGuard g(device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return launch(dev, s);
}

}  // namespace pfhe
