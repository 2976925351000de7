// The environment switches of the predict path and the choice of kernel and launch geometry for a request (gp_predict.hip launches
// what is decided here).  Host only: no kernel, no __device__ function, no HIP header -- this file is plain C++17 (it passes
// `g++ -std=c++17 -fsyntax-only -x c++`), so every threshold can be walked under a host sanitizer.
#include <cstdlib>
#include <cstring>
#include <unistd.h>
#include "predict_plan.hpp"

extern char** environ;

namespace alabi {

// Every switch of the predict path, read afresh (never cached: tests flip switches inside one process).
// ONE pass over the environment, not a getenv per switch: a per-point objective calls alabi_gp_predict for one query at a time,
// ~13 us per call, and on a host with a few hundred variables every getenv is a pass of ~0.1 us (measured: seven reads cost the
// call 0.5 us more than the three it made before they were gathered here).  As with getenv, the first entry of a name counts.
PredictSwitches predict_switches() {
    PredictSwitches sw;
    int* const flags[6] = {&sw.pm_mfma, &sw.pv_small, &sw.pv_w, &sw.pv_w2, &sw.pv_legacy, &sw.winv_dnc};
    static const char* const names[7] = {"ALABI_PM_MFMA", "ALABI_PV_SMALL", "ALABI_PV_W", "ALABI_PV_W2", "ALABI_PV_LEGACY", "ALABI_WINV_DNC",
                                         "ALABI_PV_CHUNK_TILES"};
    unsigned seen = 0;
    for (char** e = environ; e && *e; ++e) {
        if ((*e)[0] != 'A' || strncmp(*e, "ALABI_", 6) != 0) continue;
        for (int i = 0; i < 7; ++i) {
            const size_t n = strlen(names[i]);
            if ((seen >> i & 1) || strncmp(*e, names[i], n) != 0 || (*e)[n] != '=') continue;
            seen |= 1u << i;
            const char* v = *e + n + 1;
            if (i < 6) *flags[i] = (int)(unsigned char)v[0];
            else if (atoll(v) > 0) sw.pv_chunk_tiles = atoll(v);                   // tests
        }
    }
    return sw;
}

int predict_nsplit(long long tiles, int Npad, int n_cu) {
    if (tiles >= 2LL * n_cu) return 1;
    const int stages = (Npad + 255) / 256;
    int nsplit = (int)(2LL * n_cu / tiles);
    if (nsplit > stages) nsplit = stages;
    if (nsplit > 8) nsplit = 8;
    if (nsplit < 1) nsplit = 1;
    return nsplit;
}

int predict_mean_route(long long M, int d, const PredictSwitches& sw) {
    if (M >= 2048 && d + 2 <= 32 && sw.pm_mfma != '0') return PM_MFMA;
    return M <= 4096 ? PM_ROWWISE : PM_TILE;
}

MeanPlan predict_mean_plan(long long M, int Npad, int d, int n_cu, const PredictSwitches& sw) {
    MeanPlan p{predict_mean_route(M, d, sw), M, 1, 0, 0, 0};
    // d + 2 <= 32 and at least 2048 queries: the matrix-core kernel.  256-query workgroups alone fill the chip from ~200 000 queries
    // on; below that the training points are split over `parts` workgroups per query block as well, three workgroups per CU in
    // all, and mean_combine_kernel adds the parts.  Measured at N = 2000, d = 10 (vector kernels before -> now): 2048 queries
    // 28 -> 21 us, 4096 53 -> 25, 10^4 48 -> 38, 16384 63 -> 47, 32768 113 (unsplit matrix-core kernel) -> 79, 65536 192 -> 139;
    // N = 5000: 10^4 queries 104 -> 77 us; N = 10000, d = 20: 310 -> 203 us
    if (p.route == PM_MFMA) {
        p.ks = (d + 2 + 3) / 4;
        const long long wgs = (M + 255) / 256;
        p.gx = wgs;
        p.pts_per_part = Npad;
        const long long per_cu = 3;
        if (wgs < per_cu * n_cu) {
            int parts = (int)((per_cu * n_cu + wgs - 1) / wgs);
            const int tiles16 = Npad / 16;
            if (parts > tiles16 / 4) parts = tiles16 / 4;            // at least four 16-point tiles per part
            if (parts < 1) parts = 1;
            p.pts_per_part = ((tiles16 + parts - 1) / parts) * 16;
            p.parts = (Npad + p.pts_per_part - 1) / p.pts_per_part;
        }
        p.mu_stride = wgs * 256;
    } else if (p.route == PM_TILE) {
        p.gx = (M + 63) / 64;
        p.parts = predict_nsplit(p.gx, Npad, n_cu);
        p.mu_stride = p.gx * 64;
    }
    return p;
}

// Measured cross-over against the tile kernels with the split K* pre-pass: tools/prof_medium_batch.py
bool predict_var_small(long long M, int Npad, int d, const PredictSwitches& sw) {
    const long long small_max = Npad <= 2048 ? 128 : 64;
    return M <= small_max && Npad >= 256 && d <= 32 && sw.pv_small != '0';
}

VarPlan predict_var_plan(long long M, int Npad, int d, int n_cu, const PredictSwitches& sw) {
    VarPlan p{PV_FIRSTGEN, 0, 0, 0};
    // the wave-specialised kernels and the K* pre-pass exist for the dimension buckets up to 32 (dim_bucket(d) <= 32 is d <= 32)
    if (d > 32 || sw.pv_legacy == '1') {
        const long long tiles = (M + 63) / 64;
        p.grid = (int)(tiles < 512 ? tiles : 512);
        return p;
    }
    p.route = predict_use_winv(sw) ? PV_W : PV_SUBST;
    // 16-wide tiles when 64-wide ones cannot give every CU a tile
    p.TM = (M <= 16LL * n_cu) ? 16 : 64;
    // every 64-query tile owns Npad x 64 doubles of workspace (K* seeds in, V out); queries are processed in chunks so that the
    // workspace stays around 2 GiB (131072 queries at N = 2048): a whole number of rounds over the CUs (at least one round)
    long long chunk_tiles = (2LL << 30) / ((long long)Npad * 64 * 8);     // in 64-query units
    chunk_tiles = chunk_tiles / (2 * n_cu) * (2 * n_cu);      // predict_var_w2_kernel takes two tiles per workgroup
    if (chunk_tiles < 2 * n_cu) chunk_tiles = 2 * n_cu;
    if (sw.pv_chunk_tiles > 0) chunk_tiles = sw.pv_chunk_tiles;
    p.chunk = chunk_tiles * 64;
    if (p.chunk > M) p.chunk = (M + 63) / 64 * 64;
    return p;
}

VarChunk predict_var_chunk(long long mc, int Npad, int n_cu, bool use_w, int TM, const PredictSwitches& sw) {
    VarChunk c{(mc + 63) / 64, 1, false, 1, 0, 0};
    if (!use_w) {
        const long long tiles_c = (mc + TM - 1) / TM;
        c.grid_c = (int)(tiles_c < n_cu ? tiles_c : n_cu);
        return c;
    }
    // few query tiles: the K* pre-pass splits the training points over gridDim.y workgroups per tile (two of them fit on a CU)
    c.nsplit = predict_nsplit(c.groups, Npad, n_cu);
    // two MFMA waves per SIMD (128 queries per workgroup) from 2048 queries on; below that the 64-query workgroups spread over
    // more CUs (0.24 vs 0.28 ms at 256 queries, N = 2000)
    c.w2 = c.groups >= 32 && sw.pv_w2 != '0';
    const long long wgs = c.w2 ? (c.groups + 1) / 2 : c.groups;            // workgroups' worth of queries
    const int nb = Npad / 64;
    if (wgs < n_cu) { c.parts = (int)(n_cu / wgs); if (c.parts > nb) c.parts = nb; if (c.parts < 1) c.parts = 1; }
    c.gx = (int)(wgs < n_cu ? wgs : n_cu);
    return c;
}

// ---- host-only debug hook (tests/test_predict_plan_host.py): the plan of (M, N, d, n_cu) under the current environment as integers;
// returns their count.  [0, 6) the mean plan, [6] small-batch variance kernel, [7, 11) the variance plan, then six integers
// (groups, nsplit, w2, parts, gx, grid_c) for each of: the first chunk, the last chunk, the first chunk when the cached L^-1 cannot
// be had (all zero on the first-generation route); [29] L^-1 by recursive block inversion.
extern "C" int alabi_debug_predict_plan(long long M, int N, int d, int n_cu, long long* out, int cap) {
    const int Npad = (N + 63) / 64 * 64;
    const PredictSwitches sw = predict_switches();
    const MeanPlan m = predict_mean_plan(M, Npad, d, n_cu, sw);
    const VarPlan v = predict_var_plan(M, Npad, d, n_cu, sw);
    long long r[30] = {m.route, m.gx, m.parts, m.pts_per_part, m.ks, m.mu_stride, predict_var_small(M, Npad, d, sw), v.route, v.TM, v.chunk, v.grid};
    if (v.route != PV_FIRSTGEN) {
        const long long first = M < v.chunk ? M : v.chunk, last = M - (M - 1) / v.chunk * v.chunk;
        const VarChunk c[3] = {predict_var_chunk(first, Npad, n_cu, v.route == PV_W, v.TM, sw), predict_var_chunk(last, Npad, n_cu, v.route == PV_W, v.TM, sw),
                               predict_var_chunk(first, Npad, n_cu, false, v.TM, sw)};
        for (int i = 0; i < 3; ++i) {
            long long* o = r + 11 + 6 * i;
            o[0] = c[i].groups; o[1] = c[i].nsplit; o[2] = c[i].w2; o[3] = c[i].parts; o[4] = c[i].gx; o[5] = c[i].grid_c;
        }
    }
    r[29] = predict_winv_dnc(sw);
    if (out) for (int i = 0; i < 30 && i < cap; ++i) out[i] = r[i];
    return 30;
}

}  // namespace alabi
