// The environment switches of the ensemble sampler, the layout of a new handle and the choice of route, kernel blocking and chunk
// length for a run (ens_api.hip, ens_run.hip and the launchers do what is decided here).  Host only: no kernel, no __device__
// function, no HIP header -- this file is plain C++17 (it passes `g++ -std=c++17 -fsyntax-only -x c++`), so every threshold can
// be walked under a host sanitizer (tools/ens_plan_walk.cpp).
#include <cstdlib>
#include <cstring>
#include <unistd.h>
#include "ens_plan.hpp"

extern char** environ;

namespace alabi {

// Every switch of the ensemble sampler, read afresh (never cached: tests flip switches inside one process).  ONE pass over the
// environment, as predict_switches(): on a host with a few hundred variables every getenv is a pass of ~0.1 us, and a run on the
// launch-per-half-step path outside a graph used to make one per half-step launch.  As with getenv, the first entry of a name counts.
EnsSwitches ens_switches() {
    EnsSwitches sw;
    enum { NFLAG = 9, NINT = 3, NALL = 16 };
    static const char* const names[NALL] = {"STREAM", "GROUP", "GROUP_G16", "GRAPH", "MH", "MULTI", "PAIR", "PLACE", "SHARD_GRAPH",
                                            "THREADS", "GRAPH_STEPS", "SPIN_LIMIT", "CHUNK", "MH_CHUNK", "HMC_CHUNK", "NUTS_CHUNK"};
    int* const flags[NFLAG] = {&sw.stream, &sw.group, &sw.group_g16, &sw.graph, &sw.mh, &sw.multi, &sw.pair, &sw.place, &sw.shard_graph};
    int* const ints[NINT] = {&sw.threads, &sw.graph_steps, &sw.spin_limit};
    long long* const longs[NALL - NFLAG - NINT] = {&sw.chunk, &sw.mh_chunk, &sw.hmc_chunk, &sw.nuts_chunk};
    unsigned seen = 0;
    for (char** e = environ; e && *e; ++e) {
        if ((*e)[0] != 'A' || strncmp(*e, "ALABI_ENS_", 10) != 0) continue;
        const char* rest = *e + 10;
        for (int i = 0; i < NALL; ++i) {
            const size_t n = strlen(names[i]);
            if ((seen >> i & 1) || strncmp(rest, names[i], n) != 0 || rest[n] != '=') continue;
            seen |= 1u << i;
            const char* v = rest + n + 1;
            if (i < NFLAG) *flags[i] = (int)(unsigned char)v[0];
            else if (i < NFLAG + NINT) *ints[i - NFLAG] = atoi(v);
            else *longs[i - NFLAG - NINT] = atoll(v);
        }
    }
    return sw;
}

EnsCreatePlan ens_create_plan(int W, int E, int Npad, int n_cu, const EnsSwitches& sw) {
    EnsCreatePlan p{};
    // 256 compute lanes (up to 4 point pairs each) cover Npad <= 2048: few, fat waves keep the per-wave overhead of a
    // proposal (broadcast, DPP reduction) small -- measured 2.00 us per half step against 2.11 us with 512 lanes.
    // Larger training sets run on the launch-per-half-step path with 512-lane workgroups (room for several proposals per
    // workgroup in ens_half_multi_kernel).
    p.threads = (Npad / 2 <= 1024) ? 256 : 512;
    const int v = sw.threads;
    if (v == 64 || v == 128 || v == 256 || v == 512 || v == 1024) p.threads = v;
    const long long WT = (long long)W * E;
    long long cap = (4LL << 20) / WT;
    if (cap > 1024) cap = 1024;
    if (cap < 16) cap = 16;
    if (sw.chunk >= 2 && sw.chunk < cap) cap = sw.chunk;      // a shorter chunk (tests of the chunk boundary at few steps)
    p.chunk_cap = (int)cap;
    // persistent dataflow path: one workgroup per list position, all co-resident (at most one per CU): G positions-in-flight per
    // ensemble, each workgroup strides over the list
    if (E <= n_cu && !ens_stream_buffers_off(sw)) {
        int G = n_cu / E;
        if (G > (W + 1) / 2) G = (W + 1) / 2;
        p.stream_grid = G;
    }
    return p;
}

int ens_stream_ppt(const EnsShape& sh) {
    const int T = sh.threads, half = sh.Npad / 2, db = dim_bucket(sh.d);
    if (sh.d > 61 || db < 0) return 0;
    if (sh.ymap != 0) return 0;   // non-affine y scalers (pow) run on the launch-per-half-step path: this kernel has no VGPR to spare
    const int ppt = (half + T - 1) / T;
    return db <= ens_stream_max_db(T, ppt, sh.generic != 0) ? ppt : 0;
}

// G members per group: 8 for d <= 14 (rows of <= 16 words); for wider rows 8 with four point tiles per wave in registers when the
// rest of the slice then fits LDS, else 16; as many groups as the CUs allow, each with the smallest power-of-two number Q of
// 16-proposal tiles that covers its share of a half step.
GroupPlan ens_group_plan(const EnsShape& sh, int n_cu, const EnsSwitches& sw) {
    const int d = sh.d;
    GroupPlan none{};
    if (d + 2 > 32 || sh.ymap != 0 || sh.W < 2) return none;
    if (sh.E > n_cu) return none;
    const int KS = (d + 2 + 3) / 4;
    const int n0 = (sh.W + 1) / 2;
    const int tiles = sh.Npad / 16;
    for (int attempt = 0; attempt < 2; ++attempt) {
        GroupPlan pl{};
        const bool wide = KS > 4;
        if (attempt == 0 && ens_group_force_g16(sw)) continue;  // attempt 0: the instantiation with register-resident point tiles
        const int G = (wide && attempt == 1) ? 16 : 8;
        const int RT = (attempt == 0) ? ALABI_GRP_RT : 0;
        const int ng_max = n_cu / sh.E / G;
        if (ng_max < 1) continue;
        int Q = 1;
        while (Q < 8 && (n0 + 16 * Q - 1) / (16 * Q) > ng_max) Q *= 2;
        if ((n0 + 16 * Q - 1) / (16 * Q) > ng_max) continue;
        if (wide && Q > 4) continue;                         // passes of the row phase: 16 Q proposals / (8 waves x 2) <= 4
        if (!wide && RT > 0 && Q > 2) continue;              // (register budget of the narrow-row instantiations with many proposal tiles)
        pl.KS = KS; pl.Q = Q; pl.QP = 16 * Q; pl.G = G; pl.NG = (n0 + pl.QP - 1) / pl.QP; pl.RT = RT;
        pl.tpm = (tiles + G - 1) / G;
        const int tpw = (pl.tpm + ALABI_GRP_NW - 1) / ALABI_GRP_NW;
        pl.ltw = tpw > RT ? tpw - RT : 0;
        pl.lds_bytes = (size_t)group_lds(KS, pl.QP, ALABI_GRP_NW * pl.ltw).total * 8;
        pl.ok = pl.lds_bytes <= 160 * 1024 - 512;
        if (pl.ok) return pl;
    }
    return none;
}

// Steps per launch, 0 where the set does not run on this kernel.  A launch is kept to about a tenth of a second so that other
// work on the device gets its turn: a step is estimated at 3 us per tile of the training set (measured: 3.1 us for the resident
// share of ns_walk_kernel at N = 2000) times the rounds in which the E W workgroups find room (two per CU at a time), and the
// chunk is 1e5 us over that, between 64 and 16384 steps.  The step counters travel by value: the chunk length changes no result.
int ens_mh_chunk(const EnsShape& sh, int n_cu, const EnsSwitches& sw) {
    if (!sh.all_gauss || !sh.factors || sh.threads > 512 || dim_bucket(sh.d) < 0 || sh.mh_lds > ALABI_MH_MAX_LDS) return 0;
    if (ens_mh_off(sw)) return 0;
    const long long total = (long long)sh.W * sh.E;
    const long long rounds = (total + 2LL * n_cu - 1) / (2LL * n_cu);
    const long long tiles = ((sh.Npad >> 1) + sh.threads - 1) / sh.threads;
    long long chunk = 100000 / (3 * rounds * (tiles > 0 ? tiles : 1));
    if (chunk > 16384) chunk = 16384;
    if (chunk < 64) chunk = 64;
    if (sw.mh_chunk >= 1 && sw.mh_chunk < chunk) chunk = sw.mh_chunk;   // a shorter chunk (tests of the chunk boundary at few steps)
    return (int)chunk;
}

// Steps per launch, 0 where the table does not run on ens_hmc_kernel (not all HMC, no factors, a dimension without a bucket, more
// than 128 KB of LDS).  As ens_mh_chunk: a launch is kept to about a tenth of a second -- a value evaluation estimated at 3 us per
// tile of the training set, a value-and-gradient evaluation at three of those, n_leapfrog (the table's largest) of them per step,
// times the rounds in which the E W workgroups find room -- between 16 and 16384 steps.  The step counters travel by value and
// the gradient at the walker is a function of the walker alone: the chunk length changes no result.
int ens_hmc_chunk(const EnsShape& sh, int n_cu, const EnsSwitches& sw) {
    if (!sh.all_hmc || !sh.factors || dim_bucket(sh.d) < 0 || sh.hmc_lds > ALABI_HMC_MAX_LDS) return 0;
    const int T = sh.threads > 512 ? 512 : sh.threads;
    const long long total = (long long)sh.W * sh.E;
    const long long rounds = (total + 2LL * n_cu - 1) / (2LL * n_cu);
    const long long tiles = ((sh.Npad >> 1) + T - 1) / T;
    long long chunk = 100000 / (9 * rounds * (tiles > 0 ? tiles : 1) * sh.lmax);
    if (chunk > 16384) chunk = 16384;
    if (chunk < 16) chunk = 16;
    if (sw.hmc_chunk >= 1 && sw.hmc_chunk < chunk) chunk = sw.hmc_chunk;   // a shorter chunk (tests of the chunk boundary at few steps)
    return (int)chunk;
}

// Transitions per launch, 0 where the table does not run on ens_nuts_kernel (not all NUTS, no factors, a dimension without a bucket,
// more than 128 KB of LDS).  ens_hmc_chunk's estimate with the deepest tree's 2^max_depth - 1 leaves in place of n_leapfrog -- an
// estimate, not a measurement: most trees stop far short of it -- between 4 and 16384 transitions.  The counters travel by value,
// the gradient at the walker is a function of the walker alone and the per-walker sums grow transition by transition: the chunk
// length changes no result.
int ens_nuts_chunk(const EnsShape& sh, int n_cu, const EnsSwitches& sw) {
    if (!sh.all_nuts || !sh.factors || dim_bucket(sh.d) < 0 || sh.nuts_lds > ALABI_HMC_MAX_LDS) return 0;
    if (sh.lmax < 1 || sh.lmax > ALABI_NUTS_MAX_DEPTH) return 0;
    const int T = sh.threads > 512 ? 512 : sh.threads;
    const long long total = (long long)sh.W * sh.E;
    const long long rounds = (total + 2LL * n_cu - 1) / (2LL * n_cu);
    const long long tiles = ((sh.Npad >> 1) + T - 1) / T;
    long long chunk = 100000 / (9 * rounds * (tiles > 0 ? tiles : 1) * ((1LL << sh.lmax) - 1));
    if (chunk > 16384) chunk = 16384;
    if (chunk < 4) chunk = 4;
    if (sw.nuts_chunk >= 1 && sw.nuts_chunk < chunk) chunk = sw.nuts_chunk;   // a shorter chunk (tests of the chunk boundary at few steps)
    return (int)chunk;
}

// more proposals than CUs: NP per workgroup share one pass over the training set (same block size: same bits)
int ens_half_np(int threads, int d, long long total, bool hist_mode, int n_cu, const EnsSwitches& sw) {
    const int db = dim_bucket(d);
    int np = 1;
    if (threads <= 512 && db <= 24 && sw.multi != '0' && !hist_mode) {
        if (total > 3LL * n_cu && db <= 16) np = 4; else if (total > n_cu) np = 2;   // q[NP][D] lives in registers
        if (sw.multi == '4' && db <= 16) np = 4;
        if (sw.multi == '2') np = 2;
        if (sw.multi == '1') np = 1;
    }
    return np;
}

EnsRoute ens_route(const EnsShape& sh, int n_cu, const EnsSwitches& sw, bool group_allowed) {
    EnsRoute r{0, 0, false, false, false, 0};
    // An all-HMC set: ens_hmc_kernel or nothing -- there is no launch-per-half-step form, and alabi_ens_set_stream does not apply.
    if (sh.all_hmc) {
        r.chunk = ens_hmc_chunk(sh, n_cu, sw);
        r.path = r.chunk > 0 ? 5 : -1;                      // the factors and weights exceed the LDS, or no dimension bucket
        return r;
    }
    // An all-NUTS set: ens_nuts_kernel or nothing, as for HMC.
    if (sh.all_nuts) {
        r.chunk = ens_nuts_chunk(sh, n_cu, sw);
        r.path = r.chunk > 0 ? 6 : -1;
        return r;
    }
    if (sh.W < 2 && !sh.all_gauss) { r.path = -1; return r; }   // a red-blue move needs a complementary half
    // An all-Gaussian set: W independent chains, one workgroup per walker, every step of a chunk in one launch (ens_mh_kernel).
    if (sh.all_gauss && sh.mh_ok) {
        r.chunk = ens_mh_chunk(sh, n_cu, sw);
        if (r.chunk > 0) { r.path = 4; return r; }
    }
    // Which persistent kernel: ens_stream_kernel where the training set fits one workgroup's registers (N <= 2048, small d),
    // ens_group_kernel (training set partitioned over groups of workgroups, matrix-core kernel sums) beyond that;
    // ALABI_ENS_GROUP=0 disables the latter, =1 prefers it wherever its blocking is feasible.
    const bool can_stream = ens_stream_ppt(sh) > 0;
    // ens_stream_kernel takes ceil(W/2 / stream_grid) proposals per workgroup one after the other (2.0 / 3.7 / 7.1 us per half step at
    // 1 / 2 / 4 of them, N = 2000); from four on the group kernel is ahead (5.3 us at W = 2048: 1.9e8 against 1.4e8 samples/s)
    const bool crowded = can_stream && sh.stream_grid > 0 && ((sh.W + 1) / 2 + sh.stream_grid - 1) / sh.stream_grid >= 4;
    // A differential-evolution record reads two partner rows, a snooker record three: the persistent kernels hand one over, so
    // such a move set (has_de) runs with one launch per half step (and its graph replay).  Stretch-only sets differ in the draw kernel alone.
    const bool persistent = !sh.has_de && sh.stream_ok && sh.has_stream;
    const bool use_group = persistent && group_allowed && !ens_group_off(sw) && (ens_group_preferred(sw) || !can_stream || crowded) &&
                           sh.has_hist && ens_group_plan(sh, n_cu, sw).ok;
    if (persistent && (can_stream || use_group)) {
        r.path = use_group ? 3 : 1;
        if (r.path == 1) {
            // Two workgroups per list position (ens_pair_kernel) where 2 ceil(W/2) E of them fit one per CU
            const int n0 = (sh.W + 1) / 2;
            r.pair = !ens_pair_off(sw) && sh.d >= 1 && 2LL * n0 * sh.E <= n_cu;
            // Placement: both halves of a step have n0 items, n0 % 8 == 0 (whole classes), at most 128 pairs
            r.place = !ens_place_off(sw) && sh.W == 2 * n0 && n0 % 8 == 0 && n0 <= 128;
        }
        return r;
    }
    r.graph = sh.has_stream && !ens_graph_off(sw);
    r.graph_steps = sh.chunk_cap < 256 ? sh.chunk_cap : 256;
    if (sw.graph_steps > 0 && sw.graph_steps <= sh.chunk_cap) r.graph_steps = sw.graph_steps;
    return r;
}

// ---- host-only debug hook (tests/test_ens_plan_host.py, tools/ens_plan_walk.cpp): the plan of a shape under the current
// environment as integers; returns their count.  shape: the fields of EnsShape in declaration order (W, E, d, Npad, generic, ymap,
// threads, chunk_cap, stream_grid, has_hist, stream_ok, mh_ok, has_de, all_gauss, all_hmc, factors, n_moves, lmax, mh_lds, hmc_lds,
// has_stream, all_nuts, nuts_lds), missing ones as a new handle has them.  threads <= 0: the creation plan's; chunk_cap <= 0: a handle as ens_create
// leaves it -- chunk_cap and stream_grid from the creation plan, history buffers where stream_grid > 0, stream_ok only with them.
// out: [0, 3) creation plan (threads, chunk_cap, stream_grid), [3] point pairs per lane, [4, 13) group blocking (ok, Q, G, NG, RT,
// tpm, ltw, KS, LDS bytes), [13] MH chunk, [14] HMC chunk, [15, 17) proposals per workgroup of the two half-step launches of a
// step, [17, 23) route (path, chunk, pair, place, graph, graph steps), [23] path when the group kernel's buffers cannot be had,
// [24, 26) spin limit of ens_stream_kernel / ens_pair_kernel and of ens_group_kernel, [26] graph replay of the sharded run.
extern "C" int alabi_debug_ens_plan(const int* shape, int n_shape, int n_cu, long long* out, int cap) {
    enum { NSHAPE = 23, NOUT = 27 };
    EnsShape sh;
    sh.stream_ok = sh.mh_ok = sh.has_stream = 1;
    int* const f[NSHAPE] = {&sh.W, &sh.E, &sh.d, &sh.Npad, &sh.generic, &sh.ymap, &sh.threads, &sh.chunk_cap, &sh.stream_grid, &sh.has_hist,
                            &sh.stream_ok, &sh.mh_ok, &sh.has_de, &sh.all_gauss, &sh.all_hmc, &sh.factors, &sh.n_moves, &sh.lmax, &sh.mh_lds,
                            &sh.hmc_lds, &sh.has_stream, &sh.all_nuts, &sh.nuts_lds};
    for (int i = 0; shape && i < n_shape && i < NSHAPE; ++i) *f[i] = shape[i];
    if (sh.W < 1 || sh.E < 1 || sh.d < 1 || sh.Npad < 1 || n_cu < 1) return 0;
    const EnsSwitches sw = ens_switches();
    const EnsCreatePlan c = ens_create_plan(sh.W, sh.E, sh.Npad, n_cu, sw);
    if (sh.threads <= 0) sh.threads = c.threads;
    if (sh.chunk_cap <= 0) {
        sh.chunk_cap = c.chunk_cap; sh.stream_grid = c.stream_grid;
        sh.has_hist = c.stream_grid > 0;
        sh.stream_ok = sh.stream_ok && sh.has_hist;
    }
    const GroupPlan g = ens_group_plan(sh, n_cu, sw);
    const EnsRoute r = ens_route(sh, n_cu, sw), r2 = ens_route(sh, n_cu, sw, false);
    const int n0 = (sh.W + 1) / 2;
    const long long res[NOUT] = {c.threads, c.chunk_cap, c.stream_grid, ens_stream_ppt(sh),
                                 g.ok, g.Q, g.G, g.NG, g.RT, g.tpm, g.ltw, g.KS, (long long)g.lds_bytes,
                                 ens_mh_chunk(sh, n_cu, sw), ens_hmc_chunk(sh, n_cu, sw),
                                 ens_half_np(sh.threads, sh.d, (long long)n0 * sh.E, false, n_cu, sw),
                                 ens_half_np(sh.threads, sh.d, (long long)(sh.W - n0) * sh.E, false, n_cu, sw),
                                 r.path, r.chunk, r.pair, r.place, r.graph, r.graph_steps, r2.path, ens_spin_limit_stream(sw), ens_spin_limit_group(sw), ens_shard_graph_on(sw)};
    if (out) for (int i = 0; i < NOUT && i < cap; ++i) out[i] = res[i];
    return NOUT;
}

}  // namespace alabi
