// Walks the predict plan (alabi_amd/csrc/predict_plan.hip) over the sweep of tests/test_predict_plan_host.py under every switch
// value that test uses, for a host sanitizer run -- the plan is plain C++, so no GPU and no HIP is involved:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ alabi_amd/csrc/predict_plan.hip \
//       tools/predict_plan_walk.cpp -o /tmp/predict_plan_walk && /tmp/predict_plan_walk
// Prints the number of plans and a checksum of their integers; any sanitizer report ends the run with a non-zero status.
#include <cstdio>
#include <cstdlib>

extern "C" int alabi_debug_predict_plan(long long M, int N, int d, int n_cu, long long* out, int cap);

int main() {
    const char* names[] = {"ALABI_PM_MFMA", "ALABI_PV_SMALL", "ALABI_PV_W", "ALABI_PV_W2", "ALABI_PV_LEGACY", "ALABI_WINV_DNC", "ALABI_PV_CHUNK_TILES"};
    const char* values[] = {nullptr, "0", "1", "7", "66", "", "x", "-3"};
    const long long Ms[] = {1, 16, 17, 64, 65, 128, 129, 300, 2047, 2048, 2085, 4096, 4097, 5000, 16384, 65536, 300000};
    const int Ns[] = {60, 192, 300, 2000, 2100, 5000}, ds[] = {1, 4, 10, 30, 31, 40}, cus[] = {1, 64, 256, 304};
    long long plans = 0;
    unsigned long long sum = 0;
    for (const char* name : names)
        for (const char* value : values) {
            if (value) setenv(name, value, 1);
            for (long long M : Ms) for (int N : Ns) for (int d : ds) for (int n_cu : cus) {
                long long out[30];
                const int n = alabi_debug_predict_plan(M, N, d, n_cu, out, 30);
                for (int i = 0; i < n; ++i) sum = sum * 1099511628211ull + (unsigned long long)out[i];
                // a short buffer must not be overrun, a null one not be written
                long long two[2] = {-1, -1};
                if (alabi_debug_predict_plan(M, N, d, n_cu, two, 1) != n || two[1] != -1 || alabi_debug_predict_plan(M, N, d, n_cu, nullptr, 0) != n) return 1;
                ++plans;
            }
            unsetenv(name);
        }
    printf("%lld plans, checksum %016llx\n", plans, sum);
    return 0;
}
