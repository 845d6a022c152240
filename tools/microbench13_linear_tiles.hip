// microbench13_linear_tiles — which outputs-per-thread instances of lwe_linear_kernel<W, R> pay.
//
// Every R in {1, 2, 4, 8} at (in_features, out_features) = (128, 1), (128, 10), (128, 32), (128, 128), (784, 128), dimension
// 630, batch 1 and 64, u32 and u64, on the same buffers, beside the R the library's rule picks: five rounds after a
// warm-up, the instances in alternation (odd rounds in reverse order), a round being 20 launches between two device events; median per launch and spread ((max - min) / median).  Every instance must give the
// words of R = 8.  The kernels are the library's own: this unit includes csrc/pfhe_linear.hip.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-gpu-rdc -Iprimus-fhe_amd/csrc -Iinclude tools/microbench13_linear_tiles.hip \
//         -Lprimus-fhe_amd -lpfhe_hip -Wl,-rpath,'$ORIGIN/../primus-fhe_amd' -o tools/microbench13_linear_tiles
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../primus-fhe_amd/csrc/pfhe_linear.hip"

#define CHECK(x)                                                                  \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            std::printf("%s: %s\n", #x, hipGetErrorString(e_));                   \
            return 1;                                                             \
        }                                                                         \
    } while (0)

template <class W>
int run_width() {
    constexpr u32 kRow = 631, kLaunches = 20, kRounds = 5;
    const u32 shapes[5][2] = {{128, 1}, {128, 10}, {128, 32}, {128, 128}, {784, 128}};
    const int rs[4] = {1, 2, 4, 8};
    int (*const launch[4])(const W *, const W *, const W *, W *, LinearShape, hipStream_t) = {
        launch_linear_r<W, 1>, launch_linear_r<W, 2>, launch_linear_r<W, 4>, launch_linear_r<W, 8>};
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    for (const auto &shape : shapes) {
        const u32 kIn = shape[0], out_f = shape[1];
        for (u64 batch : {(u64)1, (u64)64}) {
            const size_t n_in = batch * kIn * kRow, n_w = (size_t)out_f * kIn, n_out = batch * out_f * kRow;
            std::vector<W> h(n_in + n_w + out_f);
            u64 state = 88172645463325252ull;
            for (W &v : h) {
                state ^= state << 13, state ^= state >> 7, state ^= state << 17;
                v = (W)(state * 2685821657736338717ull >> (64 - 8 * sizeof(W)));
            }
            W *d_in, *d_out[4];
            CHECK(hipMalloc(&d_in, h.size() * sizeof(W)));
            CHECK(hipMemcpy(d_in, h.data(), h.size() * sizeof(W), hipMemcpyHostToDevice));
            for (auto &o : d_out) CHECK(hipMalloc(&o, n_out * sizeof(W)));
            const W *d_w = d_in + n_in, *d_bias = d_w + n_w;
            const LinearShape sh{kRow, kIn, out_f, batch};
            std::vector<float> times[4];
            for (int i = 0; i < 4; ++i)
                if (launch[i](d_in, d_w, d_bias, d_out[i], sh, nullptr) != PFHE_OK) return 1;  // warm-up
            CHECK(hipDeviceSynchronize());
            for (u32 round = 0; round < kRounds; ++round) {
                for (int j = 0; j < 4; ++j) {
                    const int i = round % 2 ? 3 - j : j;
                    CHECK(hipEventRecord(a, nullptr));
                    for (u32 l = 0; l < kLaunches; ++l)
                        if (launch[i](d_in, d_w, d_bias, d_out[i], sh, nullptr) != PFHE_OK) return 1;
                    CHECK(hipEventRecord(b, nullptr));
                    CHECK(hipEventSynchronize(b));
                    float ms = 0;
                    CHECK(hipEventElapsedTime(&ms, a, b));
                    times[i].push_back(ms * 1e3f / kLaunches);
                }
            }
            std::vector<W> ref(n_out), got(n_out);
            CHECK(hipMemcpy(ref.data(), d_out[3], n_out * sizeof(W), hipMemcpyDeviceToHost));
            bool same = true;
            std::printf("u%zu in %3u out %3u batch %2llu picks R=%d ", 8 * sizeof(W), kIn, out_f, (unsigned long long)batch,
                        linear_rows_per_thread(sh));
            for (int i = 0; i < 4; ++i) {
                CHECK(hipMemcpy(got.data(), d_out[i], n_out * sizeof(W), hipMemcpyDeviceToHost));
                same = same && std::memcmp(got.data(), ref.data(), n_out * sizeof(W)) == 0;
                std::sort(times[i].begin(), times[i].end());
                const float med = times[i][kRounds / 2];
                std::printf(" |  R=%d %7.2f us (%4.1f %%)", rs[i], med, 100 * (times[i].back() - times[i].front()) / med);
            }
            std::printf("  |  same words %s\n", same ? "yes" : "NO");
            std::fflush(stdout);
            CHECK(hipFree(d_in));
            for (auto &o : d_out) CHECK(hipFree(o));
            if (!same) return 1;
        }
    }
    return 0;
}

int main() { return run_width<u32>() || run_width<u64>(); }
