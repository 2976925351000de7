// Hand-off latency under load: NP pairs of single-wave workgroups bounce counters through device memory at the same time
// (pair i = workgroups 2i and 2i+1, i.e. neighbouring XCDs; each pair has its own 256-byte-aligned words), optionally with
// ROWS words per message like the ensemble kernel's rows (lane k polls word k; the data is the flag).
// Pairing (first argument, "both" by default): "+1" is the above; "+8" pairs workgroup i with i + 8 inside every group of 16, which
// under round-robin dealing is the same XCD.  Every workgroup reports its HW_REG_XCC_ID, so "same XCD" is counted, not assumed.
// Build: hipcc -O3 --offload-arch=gfx950 tools/micro/pingpong_many.hip -o tools/micro/pingpong_many
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

template <int WORDS, int SHIFT, int PLUS8>
__global__ void pingpong_many(unsigned long long* buf, int rounds, int* err, int npairs, int* xcc) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int me = PLUS8 ? (i >> 3) & 1 : i & 1, pair = PLUS8 ? (i >> 4) * 8 + (i & 7) : i >> 1;
    if (pair >= npairs) return;   // "+8" rounds the grid up to whole groups of 16
    if (lane == 0) {
        int x;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x));
        xcc[2 * pair + me] = x;
    }
    unsigned long long* a = buf + (size_t)pair * 128 + SHIFT;   // 1 KB per pair: a at +SHIFT words, b 64 words further (SHIFT = 8: a 12-word row straddles two 128-byte lines)
    unsigned long long* mine = (me == 0 ? a : a + 64) + lane;
    unsigned long long* other = (me == 0 ? a + 64 : a) + lane;
    const bool act = lane < WORDS;
    for (int r = 1; r <= rounds; ++r) {
        if (me == 0 && act) __hip_atomic_store(other, (unsigned long long)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        long long spins = 0;
        while (true) {
            unsigned long long v = act ? __hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (unsigned long long)r;
            if (__all(v >= (unsigned long long)r)) break;
            if (++spins > 20000000) { *err = 1; return; }
        }
        if (me == 1 && act) __hip_atomic_store(other, (unsigned long long)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int WORDS, int SHIFT, int PLUS8>
double run(unsigned long long* buf, int npairs, int rounds, int* err, int* xcc, int* same = nullptr) {
    const int grid = PLUS8 ? (npairs + 7) / 8 * 16 : 2 * npairs;
    CK(hipMemset(buf, 0, (size_t)npairs * 1024));
    CK(hipMemset(err, 0, 4));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    hipLaunchKernelGGL((pingpong_many<WORDS, SHIFT, PLUS8>), dim3(grid), dim3(64), 0, 0, buf, 10, err, npairs, xcc);
    CK(hipDeviceSynchronize());
    CK(hipMemset(buf, 0, (size_t)npairs * 1024));
    CK(hipMemset(xcc, 0xff, 256 * sizeof(int)));
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL((pingpong_many<WORDS, SHIFT, PLUS8>), dim3(grid), dim3(64), 0, 0, buf, rounds, err, npairs, xcc);
    CK(hipEventRecord(e1));
    CK(hipDeviceSynchronize());
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    int h; CK(hipMemcpy(&h, err, 4, hipMemcpyDeviceToHost));
    if (same) {
        int x[256]; CK(hipMemcpy(x, xcc, sizeof x, hipMemcpyDeviceToHost));
        *same = 0;
        for (int p = 0; p < npairs; ++p) *same += x[2 * p] == x[2 * p + 1] && x[2 * p] >= 0;
    }
    return h ? -1.0 : 1e3 * ms / rounds / 2.0;
}

// REPS timed launches of one configuration: lowest, median and highest hop, and the pairs seen on one XCD in the last of them.
template <int WORDS, int PLUS8>
void line(unsigned long long* buf, int np, int rounds, int* err, int* xcc) {
    const int REPS = 7;
    std::vector<double> t; int same = 0;
    for (int r = 0; r < REPS; ++r) t.push_back(run<WORDS, 0, PLUS8>(buf, np, rounds, err, xcc, &same));
    std::sort(t.begin(), t.end());
    printf("%3d concurrent pairs, partner %s, %2d-word messages: one-way hop min %.3f  median %.3f  max %.3f us over %d launches; %3d of %3d pairs on one XCD\n",
           np, PLUS8 ? "+8" : "+1", WORDS, t.front(), t[REPS / 2], t.back(), REPS, same, np);
}

int main(int argc, char** argv) {
    const int rounds = 20000;
    const char* pairing = argc > 1 ? argv[1] : "both";
    int* err; CK(hipMalloc(&err, 4));
    int* xcc; CK(hipMalloc(&xcc, 256 * sizeof(int)));
    unsigned long long* buf; CK(hipMalloc(&buf, 256 * 1024));
    if (!strcmp(pairing, "+1")) {
        for (int np : {1, 8, 32, 64, 128})
            printf("%3d concurrent pairs: one-way hop %.3f us with 1-word messages, %.3f us with 12-word rows in one 128-byte line, %.3f us with rows "
                   "straddling two lines\n", np, run<1, 0, 0>(buf, np, rounds, err, xcc), run<12, 0, 0>(buf, np, rounds, err, xcc),
                   run<12, 8, 0>(buf, np, rounds, err, xcc));
        return 0;
    }
    // Placement table: the two pairings alternated at every load, so that drift over the visit hits both alike.
    for (int np : {1, 8, 32, 64, 128})
        for (int pass = 0; pass < 2; ++pass) {
            if (strcmp(pairing, "+8")) line<12, 0>(buf, np, rounds, err, xcc);
            line<12, 1>(buf, np, rounds, err, xcc);
            if (pass == 1) { if (strcmp(pairing, "+8")) line<1, 0>(buf, np, rounds, err, xcc); line<1, 1>(buf, np, rounds, err, xcc); }
        }
    return 0;
}
