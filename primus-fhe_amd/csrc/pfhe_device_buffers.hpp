// pfhe_device_buffers.hpp — the one owner of the device buffers a handle allocates at create and frees at destroy (every
// scratch-owning handle of both sides, the FFT table's twiddles, the tables of a TableSet).  Host only.
//
// The first half (BasicDeviceBuffers) needs nothing of HIP and builds with a plain host compiler against an `Env` the
// translation unit supplies (tests/test_device_buffers_cpu.py); the second half, the library's alias DeviceBuffers over
// counted_malloc / counted_free / DeviceGuard, is seen only where the HIP headers are (every source of the library).  The
// create-side recipe is DESIGN.md §16.
#pragma once

#include <cstddef>
#include <vector>

namespace pfhe {

// Env: int alloc(void **p, size_t bytes) (0 = PFHE_OK, else the status to hand on), void release(void *p), and Guard, which
// makes a device current for its scope.  bind() names the device once; with that device current, add() allocates one
// buffer per call into the handle's own typed pointer.  The object holds only what it must free, so a call never looks
// at it.  The destructor makes the bound device current itself, because a member is destroyed after the owning
// handle's destructor body (and its guard) has ended, and frees every buffer once; with nothing allocated (never bound
// included) it does nothing.
template <class Env>
class BasicDeviceBuffers {
  public:
    BasicDeviceBuffers() = default;
    BasicDeviceBuffers(const BasicDeviceBuffers &) = delete;
    BasicDeviceBuffers &operator=(const BasicDeviceBuffers &) = delete;
    ~BasicDeviceBuffers() {
        if (owned_.empty()) return;
        typename Env::Guard g(device_);
        for (void *p : owned_) Env::release(p);
    }

    void bind(int device) { device_ = device; }
    // `count` elements of *p's type in one allocation of exactly count * sizeof(T) bytes; count 0: no allocation, p stays
    // as it is (null), PFHE_OK.  A failed allocation leaves p alone and returns Env::alloc's status.
    template <class T>
    int add(T *&p, size_t count) {
        void *q = nullptr;
        const int rc = add_bytes(q, count * sizeof(T));
        if (q) p = static_cast<T *>(q);
        return rc;
    }
    // ... and of `bytes` bytes, for a buffer whose element size is decided at create
    int add(void *&p, size_t bytes) { return add_bytes(p, bytes); }
    // the sum of what was allocated
    size_t bytes() const { return bytes_; }

  private:
    int add_bytes(void *&p, size_t bytes) {
        if (!bytes) return 0;
        owned_.push_back(nullptr);  // the slot first: a buffer that exists is always on the list
        const int rc = Env::alloc(&owned_.back(), bytes);
        if (rc != 0) {
            owned_.pop_back();
            return rc;
        }
        p = owned_.back();
        bytes_ += bytes;
        return 0;
    }
    std::vector<void *> owned_;
    size_t bytes_ = 0;
    int device_ = 0;
};

}  // namespace pfhe

#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)  // the library's sources, device or host compiler
#include "pfhe_staging.hpp"

namespace pfhe {

struct HipBufferEnv {
    using Guard = DeviceGuard;
    static int alloc(void **p, size_t bytes) {
        PFHE_HIP(counted_malloc(p, bytes));
        return PFHE_OK;
    }
    static void release(void *p) { (void)counted_free(p); }
};
using DeviceBuffers = BasicDeviceBuffers<HipBufferEnv>;

}  // namespace pfhe
#endif  // __HIPCC__ || __HIP_PLATFORM_AMD__
