"""The owner of every handle's device buffers (csrc/pfhe_device_buffers.hpp), on the CPU: the HIP-free half of the header
compiled with the host compiler against a stand-in allocator that records the live pointers and the device current at
each call and can fail its j-th allocation, run plain and under AddressSanitizer + UndefinedBehaviorSanitizer.  The
failure path (allocation j of n fails) cannot be had from a real device on demand, so it is pinned here; every handle
create goes through this one class, so what holds here holds for all of them."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "primus-fhe_amd", "csrc")
SRC = r'''
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <type_traits>
#include <vector>

#include "pfhe_device_buffers.hpp"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("line %d: CHECK(%s) failed\n", __LINE__, #c); \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

// the stand-in for counted_malloc / counted_free / DeviceGuard
enum { kOk = 0, kFail = 35 };
struct Env {
    static int current;                     // the device that is current
    static int calls, fail_at, guards;      // allocation calls so far; the call to fail (1-based, 0: none); guards taken
    static std::set<void *> live;
    static std::vector<size_t> sizes;       // of every allocation that succeeded
    static std::vector<int> alloc_devices, free_devices;
    static int double_frees;
    struct Guard {
        int prev;
        explicit Guard(int device) : prev(current) { current = device, ++guards; }
        ~Guard() { current = prev; }
    };
    static int alloc(void **p, size_t bytes) {
        if (++calls == fail_at) return kFail;
        *p = std::malloc(bytes);
        live.insert(*p);
        sizes.push_back(bytes);
        alloc_devices.push_back(current);
        return kOk;
    }
    static void release(void *p) {
        free_devices.push_back(current);
        if (!live.erase(p)) {
            ++double_frees;
            return;
        }
        std::free(p);
    }
    static void reset(int fail = 0) {
        CHECK(live.empty());
        current = 0, calls = 0, fail_at = fail, guards = 0, double_frees = 0;
        sizes.clear(), alloc_devices.clear(), free_devices.clear();
    }
};
int Env::current = 0, Env::calls = 0, Env::fail_at = 0, Env::guards = 0, Env::double_frees = 0;
std::set<void *> Env::live;
std::vector<size_t> Env::sizes;
std::vector<int> Env::alloc_devices, Env::free_devices;

using Buffers = pfhe::BasicDeviceBuffers<Env>;
static_assert(!std::is_copy_constructible<Buffers>::value && !std::is_copy_assignable<Buffers>::value,
              "a copy would free every buffer twice");

// a handle as the library writes them: typed pointers, the owner as a member, a create that adds buffer after buffer
struct Handle {
    double *spec = nullptr;
    uint64_t *acc = nullptr;
    uint32_t *none = nullptr, *exps = nullptr;
    void *raw = nullptr;
    Buffers bufs;
    ~Handle() {
        Env::Guard g(7);  // the destructor body of an owner: its guard ends, another device is current again, THEN bufs dies
    }
};
constexpr int kDevice = 3, kBuffers = 4;
const size_t kSizes[kBuffers] = {5 * sizeof(double), 3 * sizeof(uint64_t), 9 * sizeof(uint32_t), 11};

#define TRY(expr)                  \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != kOk) return rc_; \
    } while (0)
static int create(Handle &h) {
    Env::Guard g(kDevice);
    h.bufs.bind(kDevice);
    TRY(h.bufs.add(h.spec, 5));
    TRY(h.bufs.add(h.acc, 3));
    TRY(h.bufs.add(h.none, 0));  // an empty buffer between the others
    TRY(h.bufs.add(h.exps, 9));
    TRY(h.bufs.add(h.raw, 11));  // the byte-counted form
    return kOk;
}

int main() {
    // n non-empty adds: n calls of the asked sizes, bytes() their sum; the empty one makes no call and leaves null
    Env::reset();
    {
        Handle h;
        CHECK(create(h) == kOk);
        CHECK(Env::calls == kBuffers && Env::sizes.size() == kBuffers && Env::live.size() == kBuffers);
        size_t sum = 0;
        for (int i = 0; i < kBuffers; ++i) {
            CHECK(Env::sizes[i] == kSizes[i] && Env::alloc_devices[i] == kDevice);
            sum += kSizes[i];
        }
        CHECK(h.bufs.bytes() == sum && h.none == nullptr);
        CHECK(h.spec && h.acc && h.exps && h.raw);
        CHECK(Env::live.count(h.spec) && Env::live.count(h.acc) && Env::live.count(h.exps) && Env::live.count(h.raw));
        h.spec[4] = 1.0, h.acc[2] = 2, h.exps[8] = 3, ((char *)h.raw)[10] = 4;  // the last element of each is the buffer's
        CHECK(Env::current == 0 && Env::free_devices.empty());                   // create's guard has ended, nothing freed yet
    }
    // after destruction: nothing live, every buffer freed once, every free under the bound device although the owner's
    // destructor body had made another one current and restored the first, and the device restored afterwards
    CHECK(Env::live.empty() && Env::double_frees == 0 && Env::free_devices.size() == kBuffers && Env::current == 0);
    for (int d : Env::free_devices) CHECK(d == kDevice);

    // allocation j of n fails, every j: the status comes back, the pointers from j on stay null, bytes() counts the
    // buffers before j, and destruction frees exactly those
    for (int j = 1; j <= kBuffers; ++j) {
        Env::reset(j);
        {
            Handle h;
            CHECK(create(h) == kFail && Env::calls == j);
            void *ptrs[kBuffers] = {h.spec, h.acc, h.exps, h.raw};
            size_t sum = 0;
            for (int i = 0; i < kBuffers; ++i) {
                CHECK((ptrs[i] != nullptr) == (i < j - 1));
                if (i < j - 1) sum += kSizes[i];
            }
            CHECK(h.none == nullptr && h.bufs.bytes() == sum && Env::live.size() == (size_t)(j - 1));
        }
        CHECK(Env::live.empty() && Env::double_frees == 0 && Env::free_devices.size() == (size_t)(j - 1));
        for (int d : Env::free_devices) CHECK(d == kDevice);
    }

    // never bound, or bound and never asked (or asked for nothing): no guard, no free
    Env::reset();
    {
        Buffers never;
        Buffers bound;
        bound.bind(kDevice);
        Buffers empty;
        uint32_t *p = nullptr;
        empty.bind(kDevice);
        CHECK(empty.add(p, 0) == kOk && p == nullptr && empty.bytes() == 0 && never.bytes() == 0);
    }
    CHECK(Env::calls == 0 && Env::guards == 0 && Env::free_devices.empty());
    std::printf("device buffers ok\n");
    return 0;
}
'''

# what a sanitizer runtime prints when it cannot start in this process (as opposed to a finding in the program)
_SAN_CANNOT_START = ("unexpected memory mapping", "failed to intercept", "runtime does not come first", "incompatible with",
                     "cannot allocate memory in static TLS", "Shadow memory range interleaves")


def _compile(d, name, extra):
    cxx = shutil.which("c++")
    assert cxx is not None, "the host compiler c++ is needed (the build uses it too)"
    src = os.path.join(d, "buffers.cpp")
    with open(src, "w") as f:
        f.write(SRC)
    exe = os.path.join(d, name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, *extra, src, "-o", exe],
                       capture_output=True, text=True)
    return exe, r


def test_owner_allocates_fails_and_frees_as_pinned():
    with tempfile.TemporaryDirectory() as d:
        exe, c = _compile(d, "buffers", [])
        assert c.returncode == 0, c.stdout + c.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "device buffers ok" in r.stdout, r.stdout + r.stderr


def test_owner_is_clean_under_address_and_ub_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe, c = _compile(d, "buffers_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
        if c.returncode != 0 and ("asan" in c.stderr or "ubsan" in c.stderr or "sanitize" in c.stderr):
            pytest.skip("the host compiler cannot link a sanitized program: " + c.stderr.strip().splitlines()[-1])
        assert c.returncode == 0, c.stdout + c.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        out = r.stdout + r.stderr
        if r.returncode != 0 and os.environ.get("LD_PRELOAD") and "device buffers ok" not in out and "CHECK(" not in out \
                and "ERROR: AddressSanitizer:" not in out and "runtime error" not in out \
                and any(m in out for m in _SAN_CANNOT_START):
            pytest.skip("the sanitizer runtime does not start under this environment's LD_PRELOAD: " +
                        out.strip().splitlines()[0])
        assert r.returncode == 0 and "device buffers ok" in r.stdout and "Sanitizer" not in out and "runtime error" not in out, out
