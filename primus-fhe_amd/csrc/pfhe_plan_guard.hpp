// pfhe_plan_guard.hpp — "one holder at a time, ordered across streams" for every handle that owns device scratch
// (external-product plans, blind-rotation handles, TFHE product plans).  Host only.
//
// The first half (PlanHold, PlanLease, PFHE_PLAN_LEASE) needs nothing of HIP and builds with a plain host compiler;
// the second half (PlanGuard, ordered_on) is seen by hipcc only.
#pragma once

#include <atomic>
#include <cstdint>

namespace pfhe {

// Exclusivity.  A handle owns the scratch of its operation (digit buffers, spectra), like the reference's
// `&mut DcrtGlevContext` (primus_lattice/src/context/glev.rs:4-10) or `&mut TfheFftContext`, which the borrow checker lets
// ONE caller hold at a time.  Here the holder is a thread: every entry point that touches the scratch takes the handle
// for the duration of the call (PlanLease), and a second thread that arrives meanwhile is refused with PFHE_ERR_BUSY
// instead of racing on the buffers.  owner = a per-thread token (0: free); depth counts nested entries of the owning
// thread (the host-pointer and profiling entry points call the device ones) and is touched by that thread only.
struct PlanHold {
    std::atomic<std::uintptr_t> owner{0};
    int depth = 0;

    static std::uintptr_t thread_token() {
        static thread_local char token;
        return reinterpret_cast<std::uintptr_t>(&token);
    }
    // take (or re-enter) the handle for the calling thread; false: another thread holds it
    bool acquire() {
        const std::uintptr_t me = thread_token();
        std::uintptr_t free_ = 0;
        if (owner.load(std::memory_order_relaxed) == me) {
            ++depth;  // nested entry of the thread that holds the handle
            return true;
        }
        if (owner.compare_exchange_strong(free_, me, std::memory_order_acquire)) {
            depth = 1;
            return true;
        }
        return false;
    }
    // undo one acquire() of the calling thread
    void release() {
        if (--depth == 0) owner.store(0, std::memory_order_release);
    }
    bool held_by_caller() const { return owner.load(std::memory_order_relaxed) == thread_token(); }
    int in_use() const { return owner.load(std::memory_order_acquire) != 0 ? 1 : 0; }
};

// the calling thread's hold on a handle for one entry point
class PlanLease {
  public:
    explicit PlanLease(PlanHold &h) : h_(h), held_(h.acquire()) {}
    ~PlanLease() {
        if (held_) h_.release();
    }
    PlanLease(const PlanLease &) = delete;
    PlanLease &operator=(const PlanLease &) = delete;
    bool held() const { return held_; }

  private:
    PlanHold &h_;
    bool held_;
};

#define PFHE_PLAN_LEASE(guard, busy_message)      \
    ::pfhe::PlanLease lease_(guard);              \
    if (!lease_.held()) {                         \
        ::pfhe::set_last_error(busy_message);     \
        return PFHE_ERR_BUSY;                     \
    }

}  // namespace pfhe

#ifdef __HIPCC__
#include "pfhe_common.hpp"

namespace pfhe {

// The hold plus the event that orders successive calls across streams.  The event belongs to `device`: init() runs with
// that device current, where the handle allocates its scratch; the destructor makes it current itself, because a
// member is destroyed after the owning handle's destructor body (and its DeviceGuard) has ended.
struct PlanGuard : PlanHold {
    hipEvent_t last_done = nullptr;  // recorded behind the last call's kernels
    bool last_valid = false;
    int device = 0;

    int init(int device_) {
        device = device_;
        PFHE_HIP(hipEventCreateWithFlags(&last_done, hipEventDisableTiming));
        return PFHE_OK;
    }
    PlanGuard() = default;
    PlanGuard(const PlanGuard &) = delete;
    PlanGuard &operator=(const PlanGuard &) = delete;
    ~PlanGuard() {
        if (!last_done) return;
        DeviceGuard g(device);
        (void)hipEventDestroy(last_done);
    }
};

// A handle's scratch is touched by `body` only.  Successive calls on DIFFERENT streams are ordered here: every call
// records the handle's `last_done` event behind its last kernel, and a call on another stream first makes that stream
// wait for it — so "one handle, used from one stream after another" needs no event handling by the caller (calls by two
// THREADS at once are refused by the lease above; work captured into a HIP graph is outside this bookkeeping: a
// capturing stream neither waits nor records, and a graph that uses a handle must not be replayed beside other users
// of it).  The result is body's.  (g.last_done is never null here: a handle whose init() failed is not handed out.)
template <class F>
int ordered_on(PlanGuard &g, hipStream_t s, F &&body) {
    const bool tracked = !stream_is_capturing(s);
    // (always, also on the stream that recorded it: a handle comparison would miss a stream destroyed and re-created at
    // the same address; waiting on one's own stream's event costs nothing)
    if (tracked && g.last_valid) PFHE_HIP(hipStreamWaitEvent(s, g.last_done, 0));
    const int rc = body();
    if (tracked) {  // also after a failed call: whatever it queued still uses the scratch
        if (hipEventRecord(g.last_done, s) == hipSuccess) {
            g.last_valid = true;
        } else {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(s);  // no event: fall back to draining the stream
            g.last_valid = false;
        }
    }
    return rc;
}

}  // namespace pfhe
#endif  // __HIPCC__
