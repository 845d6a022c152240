// pfhe_tfhe_host.hpp — the host layer under every torus entry point (pfhe_fft.hip, pfhe_bootstrap.hip, pfhe_keygen.hip,
// pfhe_pack.hip, pfhe_pack_fft.hip, pfhe_cbs.hip, pfhe_tfhe_stages.hip, pfhe_cmux.hip, pfhe_trace.hip, pfhe_lut.hip, pfhe_bitext.hip, pfhe_linear.hip, pfhe_csprng.hip): the constants and range tests they share, the launch of a
// torus kernel, and the two tails: stateless_call of the stateless steps, handle_call of the calls on a handle.  Host only.
// What is not torus-specific lives in pfhe_staging.hpp, for the RNS side too: StageBuf and stage_in / _out / _inout,
// staged_call (the staged run of a launch on host pointers), Form and form_call, refuse_null, overlaps,
// require_exps_below_2n; the lease and the stream order of a handle live in pfhe_plan_guard.hpp, and the owner of the
// device buffers a handle allocates at create in pfhe_device_buffers.hpp (the create-side recipe: DESIGN.md §16).
//
// A handle call (product, rotations, bootstrap, circuit bootstrap, CMUX and its tree, automorphism and trace, the look-up and its rotation by bits) is ONE function template for both
// of its forms:
//    1. it takes the Form (the extern "C" wrappers pass Form::kHost with a null stream, or Form::kDevice);
//    2. it refuses a null handle and takes the handle's lease (PFHE_PLAN_LEASE), once;
//    3. it runs its own checks inline, in its own order; where the two forms refuse differently (a null pointer before or
//       after the lengths, the exponents below 2N, alignment and overlap of device pointers) the line names `form`;
//    4. it returns PFHE_OK for an empty batch;
//    5. it lists its buffers as StageBufs and hands them to handle_call with the handle's guard, the table's device, the
//       stream and a callback (pointers, stream) that queues every launch of the call.
// handle_call is form_call with the launch under ordered_on: a device that cannot be made current is refused, the host form
// stages, and the launches run behind the handle's last call on whichever stream they are given.  DESIGN.md §16 lists
// every call's refusals in order.
//
// A stateless step is ONE function template for both of its forms:
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
// the gate refuses; a device that cannot be made current (form_call).  Nothing is kept between calls.
#pragma once

#include <algorithm>

#include "pfhe_fft_device.hpp"
#include "pfhe_plan_guard.hpp"
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

// ---------------- the stateless steps ----------------

struct NoGate {
    int operator()() const { return PFHE_OK; }
};

// The tail of every stateless step, values already checked and the batch not empty (the recipe is at the top of this file).
// It ends in form_call: the device form launches on the caller's pointers and stream, the host form is staged_call.
// overlap_message null: the step refuses no overlap.
template <size_t N, class Launch, class Gate = NoGate>
int stateless_call(int device, Form form, const StageBuf (&bufs)[N], const char *overlap_message, hipStream_t s,
                   Launch &&launch, Gate &&gate = Gate{}) {
    PFHE_TRY(refuse_null(bufs));
    for (size_t i = 0; overlap_message && form == Form::kDevice && i < N; ++i) {
        for (size_t j = 0; bufs[i].dir != StageBuf::kIn && j < N; ++j) {
            if (j != i && bufs[i].bytes && bufs[j].bytes && overlaps(bufs[i].host, bufs[i].bytes, bufs[j].host, bufs[j].bytes)) {
                set_last_error(overlap_message);
                return PFHE_ERR_BAD_ARGUMENT;
            }
        }
    }
    PFHE_TRY(gate());
    return form_call(device, form, bufs, s, launch);
}

// ---------------- the calls on a handle ----------------

// The tail of every handle call, the lease taken, every argument checked and the batch not empty (the recipe is at the top
// of this file): form_call whose launch runs under ordered_on(guard, ...) on the stream form_call hands it, the caller's in
// the device form and the staging context's in the host form.
template <size_t N, class Launch>
int handle_call(PlanGuard &guard, int device, Form form, const StageBuf (&bufs)[N], hipStream_t s, Launch &&launch) {
    return form_call(device, form, bufs, s, [&](void *const *d, hipStream_t st) {
        return ordered_on(guard, st, [&] { return launch(d, st); });
    });
}

}  // namespace pfhe
