// microbench14_csprng_stores — how a lane's ChaCha20 block should reach memory, and what bounds the fill.
//
// 2^26 u32 stream words from word offset 0 (so that a lane's 64 bytes are 16-byte aligned and both forms may run), four forms
// on the same buffer: five rounds after a warm-up, the forms in alternation (odd rounds in reverse order), a round being 8
// launches between two device events; median per launch and spread ((max - min) / median).
//   lds      the library's rand_fill_kernel<u32, uniform>: blocks cross LDS, a wave stores 64 consecutive words at a time
//   direct   a lane stores its own block as four 16-byte vectors (aligned offsets only: not what the library can rely on)
//   compute  the block function alone: a lane folds its block into one word and stores that (1/16 of the stores)
//   copy     hipMemcpyAsync device to device of as many bytes
// `direct` must write the words of `lds`.  The kernels under test are the library's own: this unit includes csrc/pfhe_csprng.hip.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-gpu-rdc -Iprimus-fhe_amd/csrc -Iinclude tools/microbench14_csprng_stores.hip \
//         -Lprimus-fhe_amd -lpfhe_hip -Wl,-rpath,'$ORIGIN/../primus-fhe_amd' -o tools/microbench14_csprng_stores
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../primus-fhe_amd/csrc/pfhe_csprng.hip"

#define CHECK(x)                                                  \
    do {                                                          \
        hipError_t e_ = (x);                                      \
        if (e_ != hipSuccess) {                                   \
            std::printf("%s: %s\n", #x, hipGetErrorString(e_));   \
            return 1;                                             \
        }                                                         \
    } while (0)

// block t of the stream into out[16 t .. 16 t + 15] as four 16-byte stores; blocks < n_blocks
__global__ __launch_bounds__(kThreads) void direct_kernel(RandSeed seed, uint4 *__restrict__ out, u64 n_blocks) {
    const u64 t = (u64)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_blocks) return;
    u32 x[16];
    chacha20_block(seed, t, x);
#pragma unroll
    for (int v = 0; v < 4; ++v) out[4 * t + v] = make_uint4(x[4 * v], x[4 * v + 1], x[4 * v + 2], x[4 * v + 3]);
}

__global__ __launch_bounds__(kThreads) void compute_kernel(RandSeed seed, u32 *__restrict__ out, u64 n_blocks) {
    const u64 t = (u64)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_blocks) return;
    u32 x[16], fold = 0;
    chacha20_block(seed, t, x);
#pragma unroll
    for (int j = 0; j < 16; ++j) fold ^= x[j];
    out[t] = fold;
}

int main() {
    constexpr u64 kWords = 1ull << 26, kBlocks = kWords / 16;
    constexpr int kLaunches = 8, kRounds = 5, kForms = 4;
    RandSeed seed{};
    for (u32 i = 0; i < 8; ++i) seed.key[i] = 0x03020100u + 0x04040404u * i;
    seed.nonce[0] = 7;
    u32 *a = nullptr, *b = nullptr;
    CHECK(hipMalloc(&a, kWords * 4));
    CHECK(hipMalloc(&b, kWords * 4));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const u32 groups = (u32)(kBlocks / kThreads);
    auto launch = [&](int form) -> int {
        switch (form) {
            case 0: return launch_fill<u32, kRandUniform>(seed, 0, a, kWords, 0, nullptr);
            case 1: hipLaunchKernelGGL(direct_kernel, dim3(groups), dim3(kThreads), 0, nullptr, seed, (uint4 *)b, kBlocks); return 0;
            case 2: hipLaunchKernelGGL(compute_kernel, dim3(groups), dim3(kThreads), 0, nullptr, seed, b, kBlocks); return 0;
            default: return hipMemcpyAsync(b, a, kWords * 4, hipMemcpyDeviceToDevice, nullptr) == hipSuccess ? 0 : 1;
        }
    };
    const char *names[kForms] = {"lds", "direct", "compute", "copy"};
    // the same words from both storing forms, before anything is timed
    if (launch(0) || launch(1)) return 1;
    CHECK(hipDeviceSynchronize());
    std::vector<u32> ha(kWords), hb(kWords);
    CHECK(hipMemcpy(ha.data(), a, kWords * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(hb.data(), b, kWords * 4, hipMemcpyDeviceToHost));
    std::printf("direct writes the words of lds: %s\n", ha == hb ? "yes" : "NO");
    if (ha != hb) return 1;
    for (int f = 0; f < kForms; ++f)
        if (launch(f)) return 1;  // warm-up
    CHECK(hipDeviceSynchronize());
    std::vector<float> times[kForms];
    for (int round = 0; round < kRounds; ++round) {
        for (int i = 0; i < kForms; ++i) {
            const int f = round % 2 ? kForms - 1 - i : i;
            CHECK(hipEventRecord(e0, nullptr));
            for (int l = 0; l < kLaunches; ++l)
                if (launch(f)) return 1;
            CHECK(hipEventRecord(e1, nullptr));
            CHECK(hipEventSynchronize(e1));
            float ms = 0;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            times[f].push_back(ms / kLaunches);
        }
    }
    for (int f = 0; f < kForms; ++f) {
        std::sort(times[f].begin(), times[f].end());
        const float med = times[f][kRounds / 2], spread = (times[f].back() - times[f].front()) / med;
        std::printf("u32 2^26 words  %-8s %9.1f us (%4.1f %%)  %7.1f GB/s written  %6.2f Gblock/s\n", names[f], med * 1e3, 100 * spread,
                    kWords * 4 / (med * 1e-3) / 1e9 / (f == 2 ? 16 : 1), kBlocks / (med * 1e-3) / 1e9);
    }
    CHECK(hipFree(a));
    CHECK(hipFree(b));
    return 0;
}
