"""The per-thread lease of csrc/pfhe_plan_guard.hpp (one holder at a time, re-entrant for the holder), on the CPU:
the HIP-free half of the header compiled with the host compiler and driven by two threads, plain and under
ThreadSanitizer.  Every handle that owns device scratch (external-product plans, blind-rotation handles, TFHE product
plans) takes this one lease, so what holds here holds for all of them."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "primus-fhe_amd", "csrc")
SRC = r'''
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>

#include "pfhe_plan_guard.hpp"

// what PFHE_PLAN_LEASE expects of the translation unit that uses it
enum { PFHE_OK = 0, PFHE_ERR_BUSY = 7 };
namespace pfhe {
thread_local std::string last_error;
void set_last_error(const char *m) { last_error = m; }
}  // namespace pfhe

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("line %d: CHECK(%s) failed\n", __LINE__, #c); \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

static int entry(pfhe::PlanHold &g) {  // an entry point, as the library writes them
    PFHE_PLAN_LEASE(g, "busy: held by another thread");
    return g.depth;
}

static void wait_for(const std::atomic<int> &stage, int v) {
    while (stage.load() < v) std::this_thread::yield();
}

int main() {
    pfhe::PlanHold g;
    std::atomic<int> stage{0};
    std::atomic<long> attempts{0};
    CHECK(g.in_use() == 0 && !g.held_by_caller());  // a fresh guard is free

    std::thread b([&] {
        wait_for(stage, 1);
        // A holds: no lease of B's is held, and none changes the guard
        do {
            {
                pfhe::PlanLease l(g);
                CHECK(!l.held());
            }
            CHECK(entry(g) == PFHE_ERR_BUSY && pfhe::last_error == "busy: held by another thread");
            CHECK(g.in_use() == 1 && !g.held_by_caller());
            ++attempts;
        } while (stage.load() < 2);
        stage = 3;
        wait_for(stage, 4);
        // A's outer lease has ended: B can take the guard
        {
            pfhe::PlanLease l(g);
            CHECK(l.held() && g.in_use() == 1 && g.held_by_caller() && g.depth == 1);
            CHECK(entry(g) == 2 && g.depth == 1);
            stage = 5;
            wait_for(stage, 6);
        }
    });

    {
        pfhe::PlanLease outer(g);  // thread A
        CHECK(outer.held() && g.in_use() == 1 && g.held_by_caller() && g.depth == 1);
        stage = 1;
        // nested leases of the holder, while B keeps trying
        for (int i = 0; i < 2000 || attempts.load() < 100; ++i) {
            {
                pfhe::PlanLease inner(g);
                CHECK(inner.held() && g.depth == 2);
                CHECK(entry(g) == 3);
            }
            CHECK(g.in_use() == 1 && g.held_by_caller() && g.depth == 1);  // dropping the nested one frees nothing
        }
        stage = 2;
        wait_for(stage, 3);  // B has stopped trying
        CHECK(g.in_use() == 1 && g.held_by_caller() && g.depth == 1);  // B's refused attempts changed nothing
    }
    CHECK(g.in_use() == 0 && !g.held_by_caller());  // free after the outer lease
    stage = 4;
    wait_for(stage, 5);
    // B holds now: A is the other thread
    {
        pfhe::PlanLease l(g);
        CHECK(!l.held());
    }
    CHECK(entry(g) == PFHE_ERR_BUSY && g.in_use() == 1 && !g.held_by_caller());
    stage = 6;
    b.join();
    CHECK(g.in_use() == 0);
    std::printf("lease ok after %ld refused attempts\n", attempts.load());
    return 0;
}
'''

# what a sanitizer runtime prints when it cannot start in this process (as opposed to a finding in the program)
_TSAN_CANNOT_START = ("unexpected memory mapping", "failed to intercept", "runtime does not come first",
                      "incompatible with", "cannot allocate memory in static TLS")


def _compile(d, name, extra):
    cxx = shutil.which("c++")
    assert cxx is not None, "the host compiler c++ is needed (the build uses it too)"
    src = os.path.join(d, "lease.cpp")
    with open(src, "w") as f:
        f.write(SRC)
    exe = os.path.join(d, name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror", "-I", CSRC, *extra, src, "-o", exe],
                       capture_output=True, text=True)
    return exe, r


def test_lease_one_holder_reentrant_for_its_thread():
    with tempfile.TemporaryDirectory() as d:
        exe, c = _compile(d, "lease", [])
        assert c.returncode == 0, c.stdout + c.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "lease ok" in r.stdout, r.stdout + r.stderr


def test_lease_is_clean_under_thread_sanitizer():
    with tempfile.TemporaryDirectory() as d:
        exe, c = _compile(d, "lease_tsan", ["-fsanitize=thread"])
        if c.returncode != 0 and ("tsan" in c.stderr or "sanitize" in c.stderr):
            pytest.skip("the host compiler cannot link a ThreadSanitizer program: " + c.stderr.strip().splitlines()[-1])
        assert c.returncode == 0, c.stdout + c.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        out = r.stdout + r.stderr
        if r.returncode != 0 and os.environ.get("LD_PRELOAD") and "lease ok" not in out and "CHECK(" not in out \
                and "data race" not in out and any(m in out for m in _TSAN_CANNOT_START):
            pytest.skip("the ThreadSanitizer runtime does not start under this environment's LD_PRELOAD: " +
                        out.strip().splitlines()[0])
        assert r.returncode == 0 and "lease ok" in r.stdout and "ThreadSanitizer" not in out, out
