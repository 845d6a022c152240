// pfhe_staging.cpp — per-device pool of staging contexts for the host-pointer entry points (pfhe_staging.hpp).
#include <sys/mman.h>
#include "pfhe_staging.hpp"
#include "pfhe_handles.hpp"

#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

namespace pfhe {

namespace {
std::atomic<std::uint64_t> g_alloc_events{0};

// a non-negative decimal integer, the whole value; anything else (empty, signs, trailing text, overflow) -> dflt
size_t env_bytes(const char *name, size_t dflt) {
    const char *v = std::getenv(name);
    if (!v || !*v || *v == '-' || *v == '+') return dflt;
    char *end = nullptr;
    errno = 0;
    const unsigned long long x = std::strtoull(v, &end, 10);
    return (end == v || *end != '\0' || errno == ERANGE) ? dflt : (size_t)x;
}
constexpr size_t kAlign = 256;
size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
std::atomic<std::uint64_t> g_paths[kPathCount];
}  // namespace

const StageKnobs &stage_knobs() {
    static const StageKnobs k = [] {
        StageKnobs v;
        // slices of at least register_min bytes are looked up: memory the caller pinned is used as it is
        v.use_register = true;
        v.register_min = (size_t)128 << 10;
        // transfers up to bounce_max go through the pinned bounce buffer (a CPU copy + a true asynchronous DMA, or kernels
        // on that buffer); larger ones are handed to the runtime as they are (it pins the caller's pages in pieces)
        v.bounce_max = env_bytes("PFHE_STAGE_BOUNCE_MAX", (size_t)1 << 20);
        v.cache_max = (size_t)2 << 30;
        const size_t chunk = env_bytes("PFHE_STAGE_CHUNK", 0);
        v.chunk_bytes = chunk ? chunk : (size_t)8 << 20;
        // PFHE_STAGE_ZERO_COPY=0: no kernel ever reads or writes host memory (neither the caller's pinned memory nor
        // the pool's own buffer) — every byte crosses the link through the copy engines
        v.zero_copy = env_bytes("PFHE_STAGE_ZERO_COPY", 1) != 0;
        v.helper_thread = true;
        v.pieces = 8;
        // idle contexts kept per device (each holds its arenas, up to cache_max): a burst of T concurrent callers leaves
        // at most this many behind
        v.idle_max = 4;
        // pieces the helper thread stays behind the copying thread (1: never a page in common in flight)
        v.helper_lag = 1;
        return v;
    }();
    return k;
}

void stage_path_note(StagePath which) { g_paths[which].fetch_add(1, std::memory_order_relaxed); }
std::uint64_t stage_path_count(int which) {
    return which >= 0 && which < kPathCount ? g_paths[which].load(std::memory_order_relaxed) : 0;
}

hipError_t counted_malloc(void **p, size_t bytes) {
    g_alloc_events.fetch_add(1, std::memory_order_relaxed);
    return hipMalloc(p, bytes);
}
hipError_t counted_free(void *p) {
    g_alloc_events.fetch_add(1, std::memory_order_relaxed);
    return hipFree(p);
}
hipError_t counted_host_malloc(void **p, size_t bytes) {
    g_alloc_events.fetch_add(1, std::memory_order_relaxed);
    // coherent (fine-grained): kernels read what the CPU just copied in without any cache of theirs in between
    return hipHostMalloc(p, bytes, hipHostMallocCoherent);
}
hipError_t counted_host_free(void *p) {
    g_alloc_events.fetch_add(1, std::memory_order_relaxed);
    return hipHostFree(p);
}
hipError_t counted_malloc_async(void **p, size_t bytes, hipStream_t s) {
    g_alloc_events.fetch_add(1, std::memory_order_relaxed);
    return hipMallocAsync(p, bytes, s);
}
hipError_t counted_free_async(void *p, hipStream_t s) {
    g_alloc_events.fetch_add(1, std::memory_order_relaxed);
    return hipFreeAsync(p, s);
}
std::uint64_t alloc_event_count() { return g_alloc_events.load(std::memory_order_relaxed); }

// A bump arena over a few blocks.  A call that outgrows the cached block gets a further block (earlier regions stay
// valid); when the context is returned the blocks are merged into ONE block of the bytes the call actually asked for
// (never the sum of the cached block and the overflow blocks), so the next call of the same shape allocates nothing.
// Arenas above `cache_max` are not kept.
struct Arena {
    struct Block {
        void *p;
        size_t cap;
    };
    std::vector<Block> blocks;
    size_t used = 0;    // in blocks.back()
    size_t asked = 0;   // bytes handed out during this call (rounded), over all blocks
    bool pinned = false;

    hipError_t raw_alloc(void **p, size_t bytes) const { return pinned ? counted_host_malloc(p, bytes) : counted_malloc(p, bytes); }
    void raw_free(void *p) const { (void)(pinned ? counted_host_free(p) : counted_free(p)); }
    size_t total() const {
        size_t t = 0;
        for (const Block &b : blocks) t += b.cap;
        return t;
    }
    hipError_t get(size_t bytes, void **out) {
        bytes = round_up(bytes ? bytes : 1, kAlign);
        asked += bytes;
        if (!blocks.empty() && used + bytes <= blocks.back().cap) {
            *out = static_cast<char *>(blocks.back().p) + used;
            used += bytes;
            return hipSuccess;
        }
        void *p = nullptr;
        const hipError_t e = raw_alloc(&p, bytes);
        if (e != hipSuccess) return e;
        blocks.push_back(Block{p, bytes});
        used = bytes;
        *out = p;
        return hipSuccess;
    }
    // end of a call: one block of max(cached block, bytes this call asked for) (or nothing when that exceeds cache_max)
    void recycle(size_t cache_max) {
        used = 0;
        const size_t need = asked;
        asked = 0;
        if (blocks.size() <= 1 && total() <= cache_max) return;
        const size_t want = std::max(blocks.empty() ? (size_t)0 : blocks.front().cap, need);
        for (const Block &b : blocks) raw_free(b.p);
        blocks.clear();
        if (want > cache_max) return;
        void *p = nullptr;
        if (raw_alloc(&p, want) == hipSuccess) blocks.push_back(Block{p, want});
        else (void)hipGetLastError();
    }
    void release() {
        for (const Block &b : blocks) raw_free(b.p);
        blocks.clear();
        used = asked = 0;
    }
};

struct StageCtx {
    int device = 0;
    hipStream_t s[2] = {nullptr, nullptr};
    Arena dev, pin;
    struct Pending {
        void *host;
        const void *bounce;
        size_t bytes;
    };
    std::vector<Pending> pending;
    struct Range {
        char *p;
        size_t bytes;
        bool owned;  // (always false: nothing is registered here, see HostStage::pin)
    };
    std::vector<Range> registered;  // ranges of this call that lie in memory the caller pinned
    std::vector<hipEvent_t> events;  // pooled, timing disabled
    size_t events_used = 0;

    // helper thread: parked on `cv` between tasks
    std::thread worker;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> task;
    bool has_task = false, task_done = false, quit = false;
    int task_rc = PFHE_OK;

    void worker_loop() {
        (void)hipSetDevice(device);
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return has_task || quit; });
            if (quit) return;
            std::function<int()> fn = std::move(task);
            has_task = false;
            lk.unlock();
            int rc;
            try {
                rc = fn();
            } catch (...) {
                rc = PFHE_ERR_HIP;
            }
            fn = nullptr;
            lk.lock();
            task_rc = rc;
            task_done = true;
            cv.notify_all();
        }
    }
    void stop_worker() {
        if (!worker.joinable()) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            quit = true;
        }
        cv.notify_all();
        worker.join();
    }
};

namespace {
struct Pool {
    std::mutex mu;
    std::vector<std::vector<StageCtx *>> idle;  // per device
};
// never destroyed: at process exit the HIP runtime may already be gone
Pool &pool() {
    static Pool *p = new Pool();
    return *p;
}
}  // namespace

HostStage::HostStage(int device) {
    Pool &P = pool();
    {
        std::lock_guard<std::mutex> lk(P.mu);
        if ((size_t)device < P.idle.size() && !P.idle[device].empty()) {
            ctx_ = P.idle[device].back();
            P.idle[device].pop_back();
        }
    }
    if (ctx_) return;
    auto c = std::make_unique<StageCtx>();
    c->device = device;
    c->pin.pinned = true;
    for (hipStream_t &s : c->s) {
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            for (hipStream_t t : c->s)
                if (t) (void)hipStreamDestroy(t);
            return;
        }
    }
    ctx_ = c.release();
}

// Pins [host, host + bytes) in place for this call.  Memory that already is pinned (hipHostMalloc, or registered by the
// caller) needs nothing; a refusal (read-only mapping, pages held by another registration) sends the caller to the
// bounce / pageable path.
// Memory the CALLER has pinned (hipHostMalloc, hipHostRegister, a torch pinned tensor) is copied from / to by true
// asynchronous DMA; only driver-allocated pinned memory is also handed to kernels as it is (map() below).  Pageable memory
// is NOT registered here: round 4 tried
// (hipHostRegister on the slice for the duration of the call, 1.1 us on this platform, kernels reading and writing the
// mapped range) and got rare wrong words and host-heap corruption under a debugging allocator
// (profiles/r04_experiments.txt, item 6) — pageable slices go through the pool's own pinned buffer instead.
bool HostStage::pin(const void *host, size_t bytes, bool any_size) {
    const StageKnobs &K = stage_knobs();
    char *h = static_cast<char *>(const_cast<void *>(host));
    for (const StageCtx::Range &r : ctx_->registered)
        if (h >= r.p && h + bytes <= r.p + r.bytes) return true;  // pieces of a pinned slice; in-place downloads
    if (bytes == 0 || !K.use_register || (!any_size && bytes < K.register_min)) return false;
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, h) != hipSuccess || at.type != hipMemoryTypeHost) {
        (void)hipGetLastError();
        return false;
    }
    // The whole range must lie inside ONE pinned allocation / registration: pinned first and last bytes can belong to two
    // different ones with pageable pages in between (a slice spanning two registered buffers, a partly registered array),
    // and the mapped range is handed to kernels and copy engines as a whole.  The runtime reports start and size of the
    // range that contains an address (HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR / _RANGE_SIZE: the registration's own for
    // hipHostRegister memory, where hipMemGetAddressRange returns a null base); when it cannot, or the slice sticks out of
    // it, the slice is treated as pageable.
    hipDeviceptr_t base = nullptr;
    size_t extent = 0;
    if (hipPointerGetAttribute(&base, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, h) != hipSuccess ||
        hipPointerGetAttribute(&extent, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, h) != hipSuccess || base == nullptr ||
        h < static_cast<char *>(base) || h + bytes > static_cast<char *>(base) + extent) {
        (void)hipGetLastError();
        return false;
    }
    ctx_->registered.push_back(StageCtx::Range{h, bytes, false});
    return true;
}

// Device-side address of caller memory that KERNELS may read and write in place — only memory the DRIVER allocated pinned
// (hipHostMalloc; a torch pinned tensor).  Memory that is merely REGISTERED (hipHostRegister: a userptr mapping of pages the
// host kernel still owns) is not handed to kernels: tools/microbench12_register_hazard.hip — plain HIP, no code of this
// library — registers a heap block, runs a kernel on the mapped range and unregisters it, between pageable hipMemcpy's of the
// same block, and on four MI355X hosts out of five finds 2-16 blocks in 10 000 with wrong words (part of them the values
// from before the kernel, at reused heap addresses under MALLOC_CHECK_=3); never on hipHostMalloc memory, never through the
// copy engines (profiles/r05_microbench12_register_hazard.txt).  That is round 4's "rare wrong words" (r04_experiments.txt
// item 6), reproduced this round from the caller's side inside the full test suite (tools/hazard_suite_probe.sh).
// hipHostGetFlags tells the two apart on this runtime: it succeeds for hipHostMalloc memory and fails for a registration
// (tools/probe_host_kinds.hip; every other attribute — type, device pointer, range — reads the same for both).  A registered
// slice takes the pool's own pinned buffer (short) or the copy engines (long) instead.
// The check FAILS CLOSED.  (1) The discriminator is probed once per process on a block this library registers itself: if
// hipHostGetFlags SUCCEEDS for that registration (some HIP builds report the register flags), it cannot tell the two kinds
// apart here and no caller memory is ever mapped.  (2) A second, independent property must hold as well:
// hipMemGetAddressRange reports a non-null base only for memory the driver allocated (for a registration the base is null,
// see pin()).  (3) PFHE_STAGE_ZERO_COPY=0 turns the path off altogether.
// The probe block is two pages of its OWN anonymous mapping, and it stays mapped and registered for the life of the process:
// pages that have once been registered must never come back as somebody's pageable copy source (the defect located in round
// 5 lives exactly there — profiles/r05_experiments.txt item 7), which a heap block returned to malloc would.
static bool host_flags_tell_registrations_apart() {
    static const bool works = [] {
        void *blk = mmap(nullptr, 2 * 4096, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (blk == MAP_FAILED) return false;
        if (hipHostRegister(blk, 2 * 4096, hipHostRegisterDefault) != hipSuccess) {
            (void)hipGetLastError();
            (void)munmap(blk, 2 * 4096);  // never registered: nothing to keep
            return false;
        }
        unsigned flags = 0;
        const bool ok = hipHostGetFlags(&flags, blk) != hipSuccess;  // must be refused for a registration
        (void)hipGetLastError();
        return ok;  // (the 8 KiB stay registered: see above)
    }();
    return works;
}

void *HostStage::map(void *host, size_t bytes) {
    if (!stage_knobs().zero_copy || !host_flags_tell_registrations_apart()) return nullptr;
    if (!pin(host, bytes, true)) return nullptr;
    unsigned flags = 0;
    if (hipHostGetFlags(&flags, host) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    hipDeviceptr_t base = nullptr;
    size_t extent = 0;
    if (hipMemGetAddressRange(&base, &extent, (hipDeviceptr_t)host) != hipSuccess || base == nullptr) {
        (void)hipGetLastError();
        return nullptr;
    }
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, host, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return d;
}

// a region of the pool's pinned, coherent host buffer and its device-side address
void *HostStage::bounce(size_t bytes, void **dev) {
    void *b = nullptr;
    *dev = nullptr;
    if (ctx_->pin.get(bytes, &b) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (hipHostGetDevicePointer(dev, b, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return b;
}

// true when the first or the last byte of the range is pinned memory (for a range pin() has refused: it lies PARTLY inside
// registrations; the runtime copies such a range neither as pinned nor as pageable memory — see staged_copy)
bool HostStage::touches_pinned(const void *host, size_t bytes) {
    if (bytes == 0) return false;
    const char *h = static_cast<const char *>(host);
    for (const char *p : {h, h + bytes - 1}) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost) return true;
        (void)hipGetLastError();
    }
    return false;
}

void HostStage::unpin_all() { ctx_->registered.clear(); }

int HostStage::take_event(hipEvent_t *out) {
    if (ctx_->events_used == ctx_->events.size()) {
        hipEvent_t e = nullptr;
        PFHE_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx_->events.push_back(e);
    }
    *out = ctx_->events[ctx_->events_used++];
    return PFHE_OK;
}

int HostStage::order(hipStream_t signaller, hipStream_t waiter) {
    hipEvent_t e = nullptr;
    PFHE_TRY(take_event(&e));
    PFHE_HIP(hipEventRecord(e, signaller));
    PFHE_HIP(hipStreamWaitEvent(waiter, e, 0));
    return PFHE_OK;
}

static void destroy_ctx(StageCtx *c) {
    c->stop_worker();
    DeviceGuard g(c->device);
    c->dev.release();
    c->pin.release();
    for (hipStream_t s : c->s)
        if (s) (void)hipStreamDestroy(s);
    for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
    delete c;
}

int HostStage::helper_start(std::function<int()> task, std::function<void()> on_abandon) {
    if (helper_busy_) return PFHE_ERR_BAD_ARGUMENT;
    StageCtx &c = *ctx_;
    if (!c.worker.joinable()) {
        try {
            c.worker = std::thread([ctx = ctx_] { ctx->worker_loop(); });
        } catch (...) {
            return PFHE_ERR_HIP;
        }
    }
    {
        std::lock_guard<std::mutex> lk(c.mu);
        c.task = std::move(task);
        c.has_task = true;
        c.task_done = false;
    }
    on_abandon_ = std::move(on_abandon);
    helper_busy_ = true;
    c.cv.notify_all();
    return PFHE_OK;
}

int HostStage::helper_wait() {
    if (!helper_busy_) return PFHE_OK;
    StageCtx &c = *ctx_;
    std::unique_lock<std::mutex> lk(c.mu);
    c.cv.wait(lk, [&] { return c.task_done; });
    helper_busy_ = false;
    on_abandon_ = nullptr;
    return c.task_rc;
}

HostStage::~HostStage() {
    if (!ctx_) return;
    if (helper_busy_) {  // an error path left while the helper's task may still reference the caller's frame
        if (on_abandon_) on_abandon_();
        (void)helper_wait();
    }
    if (dirty_) {
        for (hipStream_t s : ctx_->s) (void)hipStreamSynchronize(s);
        (void)hipGetLastError();
    }
    unpin_all();
    ctx_->events_used = 0;
    ctx_->pending.clear();
    const StageKnobs &K = stage_knobs();
    ctx_->dev.recycle(K.cache_max);
    ctx_->pin.recycle(K.cache_max);
    Pool &P = pool();
    StageCtx *surplus = nullptr;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        if ((size_t)ctx_->device >= P.idle.size()) P.idle.resize(ctx_->device + 1);
        // idle contexts are capped per device: a burst of concurrent callers does not pin its arenas for the life of the
        // process (StageKnobs::idle_max, four)
        if (P.idle[ctx_->device].size() < K.idle_max) P.idle[ctx_->device].push_back(ctx_);
        else surplus = ctx_;
    }
    if (surplus) destroy_ctx(surplus);
}

hipStream_t HostStage::stream() const { return ctx_->s[0]; }
hipStream_t HostStage::stream2() const { return ctx_->s[1]; }

int HostStage::alloc(size_t bytes, void **dev) {
    *dev = nullptr;
    // whoever takes arena memory is about to queue work on the context's streams: from here on every exit path — a failed
    // launch or copy included — synchronises them before the arena is recycled and the context returns to the pool
    dirty_ = true;
    PFHE_HIP(ctx_->dev.get(bytes, dev));
    return PFHE_OK;
}

int HostStage::copy_in(void *dev, const void *host, size_t bytes, hipStream_t s) {
    if (bytes == 0) return PFHE_OK;
    if (!s) s = ctx_->s[0];
    dirty_ = true;
    if (pin(host, bytes)) {
        stage_path_note(kPathDmaCaller);
        PFHE_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s));
        return PFHE_OK;
    }
    if (bytes <= stage_knobs().bounce_max) {
        stage_path_note(kPathBounceDma);
        void *b = nullptr;
        PFHE_HIP(ctx_->pin.get(bytes, &b));
        std::memcpy(b, host, bytes);
        PFHE_HIP(hipMemcpyAsync(dev, b, bytes, hipMemcpyHostToDevice, s));
        return PFHE_OK;
    }
    stage_path_note(kPathPageable);
    if (hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s) == hipSuccess) return PFHE_OK;
    (void)hipGetLastError();
    return staged_copy(dev, const_cast<void *>(host), bytes, true, s);
}

// Last resort for a range the runtime refuses to copy as one piece — a slice that lies partly inside registrations of the
// caller's (two adjacent registrations, a partly registered array) is neither pinned nor pageable to hipMemcpyAsync and comes
// back as "invalid argument": the CPU moves it through one chunk of the pool's pinned buffer at a time, synchronously.
int HostStage::staged_copy(void *dev, void *host, size_t bytes, bool to_device, hipStream_t s) {
    const size_t chunk = std::min(bytes, std::max<size_t>(stage_knobs().bounce_max, (size_t)64 << 10));
    void *b = nullptr;
    PFHE_HIP(ctx_->pin.get(chunk, &b));
    for (size_t off = 0; off < bytes; off += chunk) {
        const size_t n = std::min(chunk, bytes - off);
        if (to_device) {
            std::memcpy(b, static_cast<char *>(host) + off, n);
            PFHE_HIP(hipMemcpyAsync(static_cast<char *>(dev) + off, b, n, hipMemcpyHostToDevice, s));
            PFHE_HIP(hipStreamSynchronize(s));
        } else {
            PFHE_HIP(hipMemcpyAsync(b, static_cast<char *>(dev) + off, n, hipMemcpyDeviceToHost, s));
            PFHE_HIP(hipStreamSynchronize(s));
            std::memcpy(static_cast<char *>(host) + off, b, n);
        }
    }
    return PFHE_OK;
}

int HostStage::upload(const void *host, size_t bytes, void **dev) {
    PFHE_TRY(alloc(bytes, dev));
    return copy_in(*dev, host, bytes);
}

int HostStage::download(void *host, const void *dev, size_t bytes, hipStream_t s) {
    if (bytes == 0) return PFHE_OK;
    if (!s) s = ctx_->s[0];
    dirty_ = true;
    if (pin(host, bytes)) {
        PFHE_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
        return PFHE_OK;
    }
    if (bytes <= stage_knobs().bounce_max) {
        void *b = nullptr;
        PFHE_HIP(ctx_->pin.get(bytes, &b));
        PFHE_HIP(hipMemcpyAsync(b, dev, bytes, hipMemcpyDeviceToHost, s));
        ctx_->pending.push_back(StageCtx::Pending{host, b, bytes});
        return PFHE_OK;
    }
    if (hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s) == hipSuccess) return PFHE_OK;
    (void)hipGetLastError();
    return staged_copy(const_cast<void *>(dev), host, bytes, false, s);
}

int HostStage::finish() {
    if (!dirty_) return PFHE_OK;
    for (hipStream_t s : ctx_->s) PFHE_HIP(hipStreamSynchronize(s));
    dirty_ = false;
    unpin_all();
    for (const StageCtx::Pending &p : ctx_->pending) std::memcpy(p.host, p.bounce, p.bytes);
    ctx_->pending.clear();
    return PFHE_OK;
}

int staging_release(int device) {
    Pool &P = pool();
    std::vector<StageCtx *> victims;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        for (size_t d = 0; d < P.idle.size(); ++d) {
            if (device >= 0 && (size_t)device != d) continue;
            victims.insert(victims.end(), P.idle[d].begin(), P.idle[d].end());
            P.idle[d].clear();
        }
    }
    for (StageCtx *c : victims) destroy_ctx(c);
    return (int)victims.size();
}

// Host-pointer form of the transforms (table.rs:541-563 takes `&mut [T]` in place): the slice is staged through a
// pooled context (pfhe_staging.hpp: no allocation in steady state).  Polynomials are independent, so a long slice in
// memory the CALLER pinned is cut into pieces of whole units and pipelined over the context's two streams: one carries the
// copies in, the other waits for each piece, transforms it and copies it back — the copy back of piece i overlaps the
// copy in of piece i + 1 (the link is full duplex); pageable copies block the calling thread and go as one piece.
template <class W>
int transform_host(const TableSet &t, W *host, size_t len, bool inverse, bool lazy) {
    if (!host && len) return PFHE_ERR_BAD_ARGUMENT;
    u64 units = 0;
    PFHE_TRY(check_len(t, len, units));
    if (len == 0) return PFHE_OK;
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    HostStage st(t.device);
    if (!st.ok()) return PFHE_ERR_HIP;
    void *dv = nullptr;
    PFHE_TRY(st.alloc(len * sizeof(W), &dv));
    W *d = static_cast<W *>(dv);
    const size_t unit = t.n * t.L;
    const StageKnobs &K = stage_knobs();
    // The mapped / bounce path and the helper-thread path below exist for the u64 tables only: a u32 slice goes straight to
    // the piece loop at the end (pfhe_debug_stage_path_count stays 0 for it).
    constexpr bool kFastPaths = sizeof(W) == sizeof(u64);
    // A slice of at most one bounce buffer takes no copy engine: the CPU copies it into the pool's pinned buffer (memory
    // the caller pinned is used as it is), the kernels read and write that buffer over the link themselves (first pass
    // host -> device scratch, last pass device scratch -> host; single-pass rings in place on the mapped memory), the CPU
    // copies the result back.  Two kernel launches and one synchronisation instead of copy, two kernels, copy
    // (tools/perf_host_slice.py); PFHE_STAGE_ZERO_COPY=0 keeps the copy engines.
    if constexpr (kFastPaths) if (K.zero_copy && len * sizeof(W) <= K.bounce_max && aligned16(host)) {
        W *mapped = static_cast<W *>(st.map(host, len * sizeof(W)));
        const bool caller_mapped = mapped != nullptr;
        void *bounce = nullptr;
        if (!mapped) {
            void *bdev = nullptr;
            bounce = st.bounce(len * sizeof(W), &bdev);
            if (bounce) {
                std::memcpy(bounce, host, len * sizeof(W));
                mapped = static_cast<W *>(bdev);
            }
        }
        if (mapped) {
            const int rc = ntt_transform_through_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, mapped, d, units * t.L, inverse, lazy,
                                                     st.stream(), t.tune);
            if (rc != PFHE_ERR_UNSUPPORTED) {
                st.touch();
                stage_path_note(caller_mapped ? kPathMappedCaller : kPathMappedBounce);
                PFHE_TRY(rc);
                PFHE_TRY(st.finish());
                if (bounce) std::memcpy(host, bounce, len * sizeof(W));
                return PFHE_OK;
            }
        }
    }
    const bool pinned = st.pin(host, len * sizeof(W));
    // Long PAGEABLE slices: a pageable copy blocks the thread that issues it, so one thread alone cannot use both
    // directions of the link.  The context's HELPER THREAD (parked between calls, pfhe_staging.hpp) copies back while this
    // one copies in: the slice is cut into up to eight pieces of at least 6 MiB; this thread, piece by piece, copies in and
    // launches the transform on the context's first stream and records an event; the helper waits for each event and copies
    // that piece back on the second stream.  16 RNS polynomials of 2^16: 0.95 -> 0.79 ms, 64: 3.67 -> 2.54 ms
    // (tools/perf_host_slice.py).
    // Two rules keep the two threads apart.  (1) The helper sleeps on a condition variable until a piece is ready — no
    // spinning beside the copying thread.  (2) Adjacent pieces share the page that holds their common boundary (slices are
    // 8-byte aligned, not page aligned), and the runtime pins the caller's pages for the duration of a pageable copy: the
    // helper copies piece k back only once this thread has FINISHED copying piece k + 1 in, so the two threads never have
    // a page in common in flight (the withdrawn registration of round 4 — r04_experiments.txt item 6 — is the reason to be
    // strict about who maps the caller's pages when).
    if constexpr (kFastPaths) if (!pinned && K.helper_thread && units >= 2 && len * sizeof(W) >= ((size_t)8 << 20) &&
        !st.touches_pinned(host, len * sizeof(W))) {  // (a partly registered slice: copy_in / download stage it)
        // pieces of at least 6 MiB, at most eight (24 MiB: 2 / 3 / 4 / 6 / 8 pieces 861 / 829 / 808 / 855 / 844 us;
        // 96 MiB: 3.01 / 2.77 / 2.74 / 2.54 / 2.54 ms; one thread: 0.95 / 3.67 ms)
        const size_t pieces = std::max<size_t>(2, std::min<size_t>({K.pieces, (size_t)units, len * sizeof(W) / ((size_t)6 << 20)}));
        std::vector<hipEvent_t> done(pieces);
        for (hipEvent_t &e : done) PFHE_TRY(st.take_event(&e));
        std::vector<size_t> off(pieces + 1);
        for (size_t i = 0; i <= pieces; ++i) off[i] = (size_t)(units * i / pieces) * unit;
        // shared with the helper's task: must outlive it on EVERY exit path.  `st` was declared before these locals and is
        // therefore destroyed after them, so its destructor's own wait would come too late for an exception thrown between
        // helper_start and helper_wait: the Joiner below, declared after everything the task references, aborts and waits first.
        struct Shared {
            std::mutex mu;
            std::condition_variable cv;
            size_t copied_in = 0;  // pieces whose copy in has returned and whose transform is launched (event recorded)
            bool all_in = false, abort = false;
        } sh;
        const hipStream_t s_in = st.stream(), s_out = st.stream2();
        st.touch();
        stage_path_note(kPathHelper);
        PFHE_TRY(st.helper_start(
            [&]() -> int {
                for (size_t i = 0; i < pieces; ++i) {
                    {
                        std::unique_lock<std::mutex> lk(sh.mu);
                        // piece i is launched AND this thread's neighbour piece i + 1 is no longer being copied in
                        sh.cv.wait(lk, [&] { return sh.abort || sh.all_in || sh.copied_in >= i + 1 + K.helper_lag; });
                        if (sh.abort) return PFHE_OK;
                    }
                    hipError_t e = hipEventSynchronize(done[i]);
                    if (e == hipSuccess)
                        e = hipMemcpyAsync(host + off[i], d + off[i], (off[i + 1] - off[i]) * sizeof(W), hipMemcpyDeviceToHost, s_out);
                    if (e == hipSuccess) e = hipStreamSynchronize(s_out);
                    if (e != hipSuccess) {
                        (void)hipGetLastError();
                        return PFHE_ERR_HIP;
                    }
                }
                return PFHE_OK;
            },
            [&]() {
                std::lock_guard<std::mutex> lk(sh.mu);
                sh.abort = true;
                sh.cv.notify_all();
            }));
        struct Joiner {
            HostStage &st;
            Shared &sh;
            ~Joiner() {
                if (!st.helper_busy()) return;
                {
                    std::lock_guard<std::mutex> lk(sh.mu);
                    sh.abort = true;
                }
                sh.cv.notify_all();
                (void)st.helper_wait();
            }
        } joiner{st, sh};
        int rc = PFHE_OK;
        for (size_t i = 0; i < pieces && rc == PFHE_OK; ++i) {
            const size_t words = off[i + 1] - off[i];
            if (hipMemcpyAsync(d + off[i], host + off[i], words * sizeof(W), hipMemcpyHostToDevice, s_in) != hipSuccess) {
                rc = hip_fail(hipGetLastError(), "staged copy", __FILE__, __LINE__);
                break;
            }
            rc = transform_dev(t, d + off[i], words, inverse, lazy, s_in);
            if (rc == PFHE_OK && hipEventRecord(done[i], s_in) != hipSuccess) rc = hip_fail(hipGetLastError(), "hipEventRecord", __FILE__, __LINE__);
            if (rc == PFHE_OK) {
                std::lock_guard<std::mutex> lk(sh.mu);
                sh.copied_in = i + 1;
                sh.all_in = i + 1 == pieces;
                sh.cv.notify_all();
            }
        }
        if (rc != PFHE_OK) {
            std::lock_guard<std::mutex> lk(sh.mu);
            sh.abort = true;
            sh.cv.notify_all();
        }
        const int helper_rc = st.helper_wait();
        PFHE_TRY(rc);
        PFHE_TRY(helper_rc);
        return st.finish();
    }
    // otherwise pageable copies go as one piece (they block the calling thread: nothing to pipeline)
    const size_t per = pinned ? std::max<size_t>(1, K.chunk_bytes / (unit * sizeof(W))) : (size_t)units;
    const bool pipelined = per < units;
    const hipStream_t s_in = st.stream(), s_run = pipelined ? st.stream2() : st.stream();
    for (u64 u0 = 0; u0 < units; u0 += per) {
        const size_t words = (size_t)std::min<u64>(per, units - u0) * unit, off = (size_t)u0 * unit;
        PFHE_TRY(st.copy_in(d + off, host + off, words * sizeof(W), s_in));
        if (pipelined) PFHE_TRY(st.order(s_in, s_run));
        PFHE_TRY(transform_dev(t, d + off, words, inverse, lazy, s_run));
        PFHE_TRY(st.download(host + off, d + off, words * sizeof(W), s_run));
    }
    return st.finish();
}

template int transform_host<u64>(const TableSet &, u64 *, size_t, bool, bool);
template int transform_host<u32>(const TableSet &, u32 *, size_t, bool, bool);

}  // namespace pfhe
