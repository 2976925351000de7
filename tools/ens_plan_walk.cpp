// Walks the ensemble plan (alabi_amd/csrc/ens_plan.hip) over the sweep of tests/test_ens_plan_host.py under every switch value
// that test uses, for a host sanitizer run -- the plan is plain C++, so no GPU and no HIP is involved:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ alabi_amd/csrc/ens_plan.hip \
//       tools/ens_plan_walk.cpp -o /tmp/ens_plan_walk && /tmp/ens_plan_walk
// Prints the number of plans and a checksum of their integers; any sanitizer report ends the run with a non-zero status.
#include <cstdio>
#include <cstdlib>
#include <string>

extern "C" int alabi_debug_ens_plan(const int* shape, int n_shape, int n_cu, long long* out, int cap);

namespace {
// the handle variants of the test: ymap, threads, stream_ok, mh_ok, has_de, all_gauss, all_hmc, factors, n_moves, lmax, has_stream,
// all_nuts
const int variants[][12] = {
    {0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 1, 0},      // stretch
    {0, 0, 1, 1, 1, 0, 0, 0, 2, 1, 1, 0},      // de
    {0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0},      // gauss
    {0, 0, 1, 1, 1, 1, 0, 1, 8, 1, 1, 0},      // gauss8
    {0, 1024, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0},   // gauss_t1024
    {0, 0, 1, 0, 1, 1, 0, 1, 1, 1, 1, 0},      // gauss_mh_off
    {0, 0, 1, 1, 0, 0, 1, 1, 1, 10, 1, 0},     // hmc
    {0, 0, 1, 1, 0, 0, 1, 1, 8, 64, 1, 0},     // hmc8
    {1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 1, 0},      // ymap
    {0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 0},      // stream_off
    {0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0},      // null_stream
    {0, 0, 1, 1, 0, 0, 0, 1, 1, 8, 1, 1},      // nuts (lmax: max_depth)
    {0, 0, 1, 1, 0, 0, 0, 1, 8, 10, 1, 1},     // nuts8
};
}

int main() {
    const char* names[] = {"STREAM", "GROUP", "GROUP_G16", "GRAPH", "MH", "MULTI", "PAIR", "PLACE", "SHARD_GRAPH", "THREADS", "GRAPH_STEPS",
                           "SPIN_LIMIT", "CHUNK", "MH_CHUNK", "HMC_CHUNK", "NUTS_CHUNK"};
    const char* values[] = {nullptr, "0", "1", "2", "4", "16", "50", "64", "100", "128", "256", "512", "1000", "1024", "2000", "5000", "100000",
                            "", "x", "-3", "99999999", "99999999999999999999", "0x", "1x"};
    const int Ws[] = {1, 2, 3, 16, 17, 255, 256, 257, 2048, 8192}, Es[] = {1, 2, 8, 300}, ds[] = {1, 14, 15, 24, 25, 30, 31, 61, 62, 64};
    const int Ns[] = {60, 2000, 2100, 5000}, cus[] = {1, 64, 256, 304};
    long long plans = 0;
    unsigned long long sum = 0;
    for (const char* name : names)
        for (const char* value : values) {
            if (!value && name != names[0]) continue;              // the unset walk once
            const std::string full = std::string("ALABI_ENS_") + name;
            if (value) setenv(full.c_str(), value, 1);
            long long i = 0;
            for (int W : Ws) for (int E : Es) for (int d : ds) for (int N : Ns) for (int n_cu : cus) for (int generic = 0; generic < 2; ++generic) {
                if (i++ % 37 != 0 && value) continue;              // as the test: under a switch every 37th shape, unset all of them
                for (const auto& v : variants) {
                    const int Npad = (N + 63) / 64 * 64, nm = v[8];
                    const int shape[23] = {W, E, d, Npad, generic, v[0], v[1], 0, 0, 0, v[2], v[3], v[4], v[5], v[6], v[7], nm, v[9],
                                           nm * d * d * 8, (nm * d * (d | 1) + Npad) * 8, v[10], v[11], (nm * d * (d | 1) + Npad + 1280) * 8};
                    long long out[27];
                    const int n = alabi_debug_ens_plan(shape, 23, n_cu, out, 27);
                    if (n != 27) return 2;
                    for (int k = 0; k < n; ++k) sum = sum * 1099511628211ull + (unsigned long long)out[k];
                    // a short buffer must not be overrun, a null one not be written, a short shape is completed with defaults
                    long long two[2] = {-1, -1};
                    if (alabi_debug_ens_plan(shape, 21, n_cu, two, 1) != n || two[1] != -1 || alabi_debug_ens_plan(shape, 4, n_cu, nullptr, 0) != n) return 1;
                    ++plans;
                }
            }
            unsetenv(full.c_str());
        }
    printf("%lld plans, checksum %016llx\n", plans, sum);
    return 0;
}
