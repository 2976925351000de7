// The task lists of the queue factorisation (chol_queue.hpp runs them, gp_cholesky.hip launches them) and the environment switches
// of the whole Cholesky.  Host only: no kernel, no __device__ function, no HIP header -- this file is plain C++17 (it passes
// `g++ -std=c++17 -fsyntax-only -x c++`), so the combinatorics can be built and run under a host sanitizer.
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>
#include "chol_tasks.hpp"

namespace alabi {

// Every switch of the factorisation, read afresh (never cached: tests flip switches inside one process).
CholSwitches chol_switches() {
    auto flag = [](const char* name) { const char* e = getenv(name); return e ? (int)(unsigned char)e[0] : CHOL_UNSET; };
    auto number = [](const char* name, int lo, int hi, int* out) { if (const char* e = getenv(name)) { const int v = atoi(e); if (v >= lo && v <= hi) *out = v; } };
    CholSwitches sw;
    number("ALABI_CHOL_GK", 1, 64, &sw.list.gk);
    number("ALABI_CHOL_NEAR", 1, 16, &sw.list.near);
    sw.list.w8 = flag("ALABI_CHOL_W8");
    sw.list.update2 = flag("ALABI_CHOL_UPDATE2");
    sw.list.update4 = flag("ALABI_CHOL_UPDATE4");
    number("ALABI_BATCH_GK", 1, 255, &sw.list.batch_gk);
    sw.list.batch_left = flag("ALABI_BATCH_LEFT");
    sw.list.batch_phases = flag("ALABI_BATCH_PHASES");
    sw.tasks = flag("ALABI_CHOL_TASKS");
    number("ALABI_CHOL_SPIN_LIMIT", 1, 0x7fffffff, &sw.spin_limit);
    if (const char* e = getenv("ALABI_CHOL_PANEL")) { const int v = atoi(e); if (v == 0 || v == 2 || v == 4 || v == 6 || v == 8) sw.panel = v; }
    sw.lookahead = flag("ALABI_CHOL_LOOKAHEAD");
    sw.log_print = getenv("ALABI_CHOL_LOG_PRINT") != nullptr;
    number("ALABI_BATCH_LISTS", 1, 8, &sw.batch_lists);
    number("ALABI_BATCH_WINDOW", 0, 4096, &sw.batch_window);
    return sw;
}

// Task list of the queue kernel for nb block columns: a static topological order, drawn from one counter.
//   step k (block column k is final once its tasks are done):
//     CHAIN(k+1)                      solve tile (k+1,k), update and factorise tile (k+1,k+1), all in one workgroup
//     TRSM(i,k), i >= k+2             the rest of panel k
//     UPDATE(i,j,k) with ONE block column for the tile columns j = k+1 (inputs of CHAIN(k+2) and of panel k+1) .. k+near
//     UPDATE(i,j,[far(j), k]) for tile column j = k+1+near: everything it has not received yet, in one task
//     UPDATE(i,j,[k+1-gk, k]) for the tile columns beyond, whenever a group of gk block columns is complete
//   far(j) = gk * floor((j - near) / gk) (0 below).  A tile far from the chain takes the block columns in groups of gk -- C is
//   read and written once per group instead of once per block column, and a task carries gk x 64 matrix-core instructions per wave
//   against its fixed cost (queue draw, dependency poll, first fetch, C round trip: 3.5 us against 2.7 us per block column) --,
//   catches up in one task when the chain is near + 1 columns away, and from then on takes every block column as soon as it is
//   final, so that nothing the chain needs waits for a group to fill.
// Every task depends only on tasks before it in the list (tests/test_abi.py replays the order on the host).
// (Round 3, measured and not kept: a batch of grouped updates dealt over the following gk steps -- a share per step, in front of or
// behind its one-column updates, each column's share flushed before anything else touches the column -- so that the one-column
// tasks find their panel tiles solved instead of waiting 4.4 us each: N = 3072 0.84 -> 0.81 ms, but 8192 5.0 -> 5.55 and 10000
// 8.1 -> 8.6-8.7 either way; a batch in one piece keeps the operand tiles of a tile column in the XCDs' L2s while they are used.)
static void chol_build_tasks(int nb, int gk, int near, bool two, bool four, std::vector<CholTask>& t) {
    // four: 2 x 2 tiles per grouped update from ALABI_CHOL_UPDATE4_MIN_NB block columns on (measured: N = 3072 0.87 -> 0.94 ms, 5000 1.82 -> 1.88,
    // 8192 5.09 -> 4.97, 10000 8.36 -> 8.13, 16000 28.9 -> 27.5: the big tasks pay when the trailing matrix is wide)
    four = four && two;
    auto far = [&](int j) { return (j - near) < 0 ? 0 : (j - near) / gk * gk; };
    t.clear();
    t.push_back({0, 0, 0, 0});
    for (int k = 0; k + 1 < nb; ++k) {
        t.push_back({0, k + 1, k + 1, k + 1});
        for (int i = k + 2; i < nb; ++i) t.push_back({1, i, k, k});
        for (int i = k + 2; i < nb; ++i) t.push_back({2 | (1 << 8), i, k + 1, k});
        for (int j = k + 2; j < nb && j <= k + near; ++j)
            for (int i = j; i < nb; ++i) t.push_back({2 | (1 << 8), i, j, k});
        const int jc = k + 1 + near;                          // catches up: block columns [far(jc), k]
        if (jc < nb && far(jc) <= k)                          // (one tile per task: as UPDATE2 pairs these cost 6 % at N = 10000 -- the chain is near)
            for (int i = jc; i < nb; ++i) t.push_back({2 | ((k + 1 - far(jc)) << 8), i, jc, far(jc)});
        if ((k + 1) % gk == 0)
            for (int j = k + 1 + near; j < nb; ++j) {
                if (far(j) < k + 1) continue;                 // (j = k+1+near has far(j) = k+1 here: its catch-up task above is empty)
                const int k0 = k + 1 - gk;
                if (four && j + 1 < nb) {
                    // tile columns j and j + 1 together: the diagonal tile (j, j) alone, then 2 x 2 blocks of tiles from row j + 1 on
                    t.push_back({2 | (gk << 8), j, j, k0});
                    int i = j + 1;
                    for (; i + 1 < nb; i += 2) t.push_back({5 | (gk << 8), i, j, k0});
                    if (i < nb) { t.push_back({2 | (gk << 8), i, j, k0}); t.push_back({2 | (gk << 8), i, j + 1, k0}); }
                    ++j;
                    continue;
                }
                for (int i = j; i < nb; ++i) {
                    if (two && i + 1 < nb) { t.push_back({4 | (gk << 8), i, j, k0}); ++i; }            // tiles (i, j) and (i + 1, j)
                    else t.push_back({2 | (gk << 8), i, j, k0});
                }
            }
    }
}

// The list for a matrix that shares the queue with many others (chol_batch_build).  There the chip is kept busy by the OTHER
// matrices, so nothing has to be fed to a matrix's own chain early and no tile takes a block column on its own: every tile receives
// full groups of gk block columns while the chain is far, and ONE catch-up task brings it up to date at the last moment --
//   off-diagonal (i, j): at step j - 1 (then TRSM(i, j) / CHAIN(j) can solve it), diagonal (j, j): at step j - 2 (CHAIN(j) applies
//   column j - 1 itself); the catch-up covers [gk floor(c / gk), c] for catch-up step c, the groups before it are complete.
// With gk >= nb this is the left-looking factorisation: every tile is read and written once.  Against the list above (near = 4):
// 276 single-column tasks fewer per matrix of 25 block columns, each of which paid a task's fixed cost (queue draw, dependency
// poll, first fetch, C round trip) for 64 matrix-core instructions per wave.  Every tile still receives its block columns in
// ascending order inside register accumulators: the same bits.
static void chol_build_tasks_batch(int nb, int gk, bool two, bool four, std::vector<CholTask>& t) {
    t.clear();
    t.push_back({0, 0, 0, 0});
    auto grouped = [&](int j, int i0, int cnt, int k0) {                 // tiles (i, j), i = i0 .. nb - 1, block columns k0 .. k0 + cnt - 1
        for (int i = i0; i < nb; ++i) {
            if (two && cnt >= 2 && i + 1 < nb) { t.push_back({4 | (cnt << 8), i, j, k0}); ++i; }
            else t.push_back({2 | (cnt << 8), i, j, k0});
        }
    };
    for (int k = 0; k + 1 < nb; ++k) {
        t.push_back({0, k + 1, k + 1, k + 1});
        for (int i = k + 2; i < nb; ++i) t.push_back({1, i, k, k});
        const int c0 = k / gk * gk, cc = k + 1 - c0;                      // catch-ups of this step: block columns [c0, k]
        grouped(k + 1, k + 2, cc, c0);                                    // column k + 1 below its diagonal tile
        if (k + 2 < nb) t.push_back({2 | (cc << 8), k + 2, k + 2, c0});   // diagonal tile (k + 2, k + 2)
        if ((k + 1) % gk == 0) {                                          // a group is complete: everything whose catch-up is still ahead
            const int k0 = k + 1 - gk;
            grouped(k + 2, k + 3, gk, k0);                                // column k + 2 without its diagonal tile (caught up above)
            for (int j = k + 3; j < nb; ++j) {
                if (four && gk >= 2 && j + 1 < nb) {                      // tile columns j and j + 1: (j, j) alone, then 2 x 2 blocks
                    t.push_back({2 | (gk << 8), j, j, k0});
                    int i = j + 1;
                    for (; i + 1 < nb; i += 2) t.push_back({5 | (gk << 8), i, j, k0});
                    if (i < nb) { t.push_back({2 | (gk << 8), i, j, k0}); t.push_back({2 | (gk << 8), i, j + 1, k0}); }
                    ++j;
                    continue;
                }
                grouped(j, j, gk, k0);
            }
        }
    }
}

// Block columns per far update and width of the near band, by size: measured in tools/prof_cholesky.py
static void chol_task_shape(int nb, const CholListShape& sh, int* gk, int* near) {
    // measured (profiles/r03_cholesky_task_shapes.txt): N = 2000: (4,4) 0.585 ms, (8,4) 0.578, (16,3) 0.627; N = 3072: (4,2) 0.98,
    // (16,3) 0.96; N = 5000: (4,2) 2.18, (8,4) 2.06, (16,4) 1.98; N = 8192: (16,3) 5.87, (32,3) 6.19; N = 10000: (8,2) 10.3, (16,3) 9.91
    *gk = nb < 40 ? 4 : nb < 64 ? 8 : 16; *near = nb < 100 ? 4 : 3;
    if (sh.gk != 0) *gk = sh.gk;
    if (sh.near != 0) *near = sh.near;
}

bool chol_tasks_w8(int nb, const CholListShape& sh) {     // eight waves per workgroup (chol_tasks8_kernel)?
    return sh.w8 == CHOL_UNSET ? nb >= ALABI_CHOL_W8_MIN_NB : sh.w8 == '1';
}
static bool chol_tasks_two(int nb, int gk, const CholListShape& sh) {   // grouped updates of two tiles per task (UPDATE2; eight-wave kernel, gk >= 2)
    return chol_tasks_w8(nb, sh) && gk >= 2 && sh.update2 != '0';
}

void chol_single_tasks(int nb, const CholListShape& sh, std::vector<CholTask>& t) {
    int gk, near;
    chol_task_shape(nb, sh, &gk, &near);
    chol_build_tasks(nb, gk, near, chol_tasks_two(nb, gk, sh), chol_four_single(sh, nb), t);
}

// ---------------------------------------------------------------------------------------------------------------------
// Batched task queue: B independent matrices in ONE launch (gp_batch.hip: the folds x candidates of the hyper-parameter search).
// A single matrix of 16..40 block columns leaves the chip idle -- its time is the chain of nb CHAIN tasks, ~17 us each, with 8 %
// matrix-core duty at N = 2000 -- so the task lists of many matrices are interleaved: the chains of different matrices run side by
// side on different workgroups and the bulk updates of one fill the gaps of another.
//   * matrix b goes to list b % nlists (one list per XCD: its tiles stay in that XCD's L2, its own head counter);
//   * inside a list the matrices advance in SLOTS: slot t holds step t - start_m of every matrix m of the list that is active,
//     start_m = floor(rank_m * stagger) -- with stagger = steps / P about P matrices per list are in flight at any time, in
//     different phases (the wide early steps of one beside the narrow late steps of another), and the working set stays
//     ~ P * nlists lower triangles instead of all B;
//   * within a slot the matrices closest to their end come first (their steps are short and chain-bound).
// Each matrix keeps the order of its own list, so every list remains a topological order.
// (Round 4, measured and not kept -- tools/experiments/chol_batch_trsm3_tasks.patch: two or three panel tiles per TRSM task, one wave's
// slab recurrence per tile side by side, bit-identical: 500 matrices of N = 1600 28.5-29.2 ms with one tile per task in that build,
// 27.6-27.9 with two / three -- but the build without the extra task type does 27.5-28.0: the new code path costs the kernel 15 more
// spilled registers, which takes back what the TRSM tasks gain; N = 8000 4.50 -> 4.38 ms per fit.)
// ALABI_BATCH_GK: block columns per group, ALABI_BATCH_LEFT=0: the single-matrix list instead.  Measured (tools/prof_batch_cv.py, 500
// matrices of N = 1600 per call, everything included): the single-matrix list 46.6 ms; this one 34.3 (gk 4), 31.9 (8), 31.8 (10), 32.1 (12),
// 35.5 (16), 36.9 (32 = left-looking) -- profiles/r04_batch_sweeps.txt
static void chol_batch_shape(int nb, const CholListShape& sh, std::vector<CholTask>& t) {
    if (chol_batch_left(sh)) chol_build_tasks_batch(nb, sh.batch_gk, true, chol_four_batch(sh), t);
    else chol_single_tasks(nb, sh, t);
}
int chol_batch_build(const std::vector<int>& nbs, int nlists, int window, const CholListShape& sh, std::vector<CholTask>& out,
                     std::vector<int>& list_off) {
    std::map<int, std::pair<std::vector<CholTask>, std::vector<int>>> per_nb;       // nb -> (tasks, first task of every step)
    for (int nb : nbs) {
        if (per_nb.count(nb)) continue;
        auto& e = per_nb[nb];
        chol_batch_shape(nb, sh, e.first);
        for (size_t q = 0; q < e.first.size(); ++q)
            if ((e.first[q].type & 255) == 0) e.second.push_back((int)q);            // a CHAIN task opens a step
        e.second.push_back((int)e.first.size());
    }
    out.clear();
    list_off.assign(nlists + 1, 0);
    for (int q = 0; q < nlists; ++q) {
        list_off[q] = (int)out.size();
        std::vector<int> mem;                                                        // matrices of this list
        for (int b = q; b < (int)nbs.size(); b += nlists) mem.push_back(b);
        if (mem.empty()) continue;
        std::vector<int> start(mem.size());
        int last_slot = 0;
        for (size_t r = 0; r < mem.size(); ++r) {
            const int steps = nbs[mem[r]];
            const double stagger = window > 0 ? (double)steps / window : 0.0;
            start[r] = (int)(r * stagger);
            if (start[r] + steps > last_slot) last_slot = start[r] + steps;
        }
        // Inside a slot the tasks go PHASE by phase over the active matrices -- every matrix's CHAIN, then every matrix's panel solves,
        // then every matrix's catch-up updates (what the NEXT step's CHAIN and panel solves read), then every matrix's grouped updates
        // -- not matrix by matrix: the updates of a step wait for the CHAIN and the panel solves of the SAME step, drawn moments before
        // them, and the next CHAIN waits for this step's catch-ups; with the other matrices' tasks in between, a task's inputs are
        // finished when a workgroup reaches it instead of holding that workgroup for up to a CHAIN's 17 us (ALABI_BATCH_PHASES=0:
        // matrix by matrix; =3: without the split of the updates).  A matrix's own tasks keep their order (its step is CHAIN, panel
        // solves, catch-ups, groups in that order already).
        const int nphase = sh.batch_phases == '0' ? 1 : (sh.batch_phases == '3' || !chol_batch_left(sh)) ? 3 : 4;
        for (int t = 0; t < last_slot; ++t)
            for (int phase = 0; phase < nphase; ++phase)
                for (size_t r = 0; r < mem.size(); ++r) {                           // lower rank = started earlier = closer to its end
                    const int b = mem[r], st = t - start[r];
                    if (st < 0 || st >= nbs[b]) continue;
                    const auto& e = per_nb[nbs[b]];
                    for (int x = e.second[st]; x < e.second[st + 1]; ++x) {
                        CholTask c = e.first[x];
                        const int ty = c.type & 255, k = st - 1;                    // step st factorises block column k + 1 = st
                        int ph = ty == 0 ? 0 : ty == 1 ? 1 : 2;
                        if (ph == 2 && nphase == 4 && !(c.j == k + 1 || (c.i == c.j && c.j == k + 2))) ph = 3;   // not a catch-up: a grouped update
                        if (nphase > 1 && ph != phase) continue;
                        c.type |= b << 16;
                        out.push_back(c);
                    }
                }
    }
    list_off[nlists] = (int)out.size();
    return (int)out.size();
}

// ---- host-only debug hooks (tests/test_abi.py, tests/test_chol_task_lists_pinned.py): the lists as (type, i, j, k) quadruples; return the count
static int chol_tasks_out(const std::vector<CholTask>& t, int* out, int cap) {
    if (out)
        for (size_t q = 0; q < t.size() && (int)q < cap; ++q) { out[4 * q] = t[q].type; out[4 * q + 1] = t[q].i; out[4 * q + 2] = t[q].j; out[4 * q + 3] = t[q].k; }
    return (int)t.size();
}
extern "C" int alabi_debug_chol_tasks(int nb, int* out, int cap) {
    std::vector<CholTask> t;
    chol_single_tasks(nb, chol_switches().list, t);
    return chol_tasks_out(t, out, cap);
}
extern "C" int alabi_debug_chol_batch_matrix_tasks(int nb, int* out, int cap) {   // ONE matrix's list inside a batch
    std::vector<CholTask> t;
    chol_batch_shape(nb, chol_switches().list, t);
    return chol_tasks_out(t, out, cap);
}
extern "C" int alabi_debug_chol_batch_tasks(int B, const int* nbs, int nlists, int window, int* out, int cap, int* list_off_out) {
    std::vector<int> v(nbs, nbs + B), lo;
    std::vector<CholTask> t;
    chol_batch_build(v, nlists, window, chol_switches().list, t, lo);
    if (list_off_out) for (int q = 0; q <= nlists; ++q) list_off_out[q] = lo[q];
    return chol_tasks_out(t, out, cap);
}

}  // namespace alabi
