// empty_launch_probe.hip -- what a chained step costs when its kernel finds nothing to do: `grid` workgroups of
// 256 threads that read one word and return, `launches` of them back to back alternating between two
// non-blocking streams (the chain's two sides), timed with a HIP event pair around the whole batch (the second
// stream joins the first before the closing event).  Also the same batch on one stream, for the price of the
// alternation itself.  Prints one JSON line per (mode, round): us per launch.
// Build: hipcc -O3 --offload-arch=gfx950 -o empty_launch_probe tools/empty_launch_probe.hip
// Run:   empty_launch_probe [grid=508] [launches=200] [rounds=5]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                                                           \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                        \
            exit(1);                                                                       \
        }                                                                                  \
    } while (0)

__global__ __launch_bounds__(256) void empty_step(const unsigned long long *word, unsigned long long *out) {
    if (*word == ~0ull) out[0] = 1ull;   // never true: the word is 0
}

int main(int argc, char **argv) {
    const int grid = argc > 1 ? atoi(argv[1]) : 508;
    const int launches = argc > 2 ? atoi(argv[2]) : 200;
    const int rounds = argc > 3 ? atoi(argv[3]) : 5;
    if (grid < 1 || grid > 65536 || launches < 1 || launches > 100000 || rounds < 1 || rounds > 100) {
        fprintf(stderr, "usage: empty_launch_probe [grid 1..65536] [launches 1..100000] [rounds 1..100]\n");
        return 2;
    }
    unsigned long long *d = nullptr;
    CHECK(hipMalloc(&d, 2 * sizeof(unsigned long long)));
    CHECK(hipMemset(d, 0, 2 * sizeof(unsigned long long)));
    hipStream_t s[2];
    for (auto &x : s) CHECK(hipStreamCreateWithFlags(&x, hipStreamNonBlocking));
    hipEvent_t e0, e1, fork, join;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    CHECK(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
    CHECK(hipEventCreateWithFlags(&join, hipEventDisableTiming));
    auto batch = [&](bool two) -> double {
        CHECK(hipEventRecord(e0, s[0]));
        if (two) {
            CHECK(hipEventRecord(fork, s[0]));
            CHECK(hipStreamWaitEvent(s[1], fork, 0));
        }
        for (int k = 0; k < launches; ++k)
            hipLaunchKernelGGL(empty_step, dim3(grid), dim3(256), 0, s[two ? k & 1 : 0], d, d + 1);
        CHECK(hipGetLastError());
        if (two) {
            CHECK(hipEventRecord(join, s[1]));
            CHECK(hipStreamWaitEvent(s[0], join, 0));
        }
        CHECK(hipEventRecord(e1, s[0]));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        return ms * 1e3 / launches;
    };
    for (int two = 0; two < 2; ++two) batch(two != 0);   // untimed: code objects loaded, queues made
    for (int r = 0; r < rounds; ++r)
        for (int two = 0; two < 2; ++two) {
            printf("{\"mode\": \"%s\", \"grid\": %d, \"launches\": %d, \"round\": %d, \"us_per_launch\": %.3f}\n",
                   two ? "two_streams" : "one_stream", grid, launches, r, batch(two != 0));
            fflush(stdout);
        }
    CHECK(hipDeviceSynchronize());
    CHECK(hipFree(d));
    return 0;
}
