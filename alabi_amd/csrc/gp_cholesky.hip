// Blocked right-looking Cholesky (lower, in place, fp64) for gfx950: the launchers of its three paths.
//
// Replaces scipy.linalg.cholesky inside george's BasicSolver.compute, reached from the
// reference at alabi/core.py:1158 (every active-learning iteration), :1430, :1577 and
// alabi/gp_utils.py:243.  Work: N^3/3 flops on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), 64 x 64 tiles staged in LDS.
// The matrix is [Npad, Npad] row-major with identity padding, so every block is full; a non-positive pivot is reported as
// LAPACK's potrf `info` (1-based) on every path.
//
//   task queue        ONE launch: the tile operations are tasks in a static topological order that persistent workgroups draw from an
//   (the default for  atomic counter.  cholesky_tasks_prepare / launch_cholesky_tasks here; device code and protocol in chol_queue.hpp;
//   3..256 block      the lists and their order in chol_tasklist.hip.  A wait that runs out sets a flag and the caller (api.hip)
//   columns)          assembles and factorises again on the launch-per-step path.
//   launch per step   Two launches per 64-column block step (panel solve; trailing update with the next diagonal factorisation fused
//   (below 3 and      in), from 110 block columns on in panels of 8 with one rank-512 update behind each and look-ahead on a second stream.
//   above 256 block   launch_cholesky_steps / launch_cholesky here; the kernels in chol_steps.hpp.
//   columns, forced
//   off, fallback)
//   batched queue     Many independent matrices in one launch of the queue kernel (gp_batch.hip: the folds x candidates of the
//                     hyper-parameter search).  chol_batch_prepare / _launch / _free here; chol_batch_build in chol_tasklist.hip.
//
// All DEVICE code of the three paths is compiled in this one translation unit, in the order tiles, step kernels, queue: the code
// generated for these kernels depends on which other kernels share their module and in which order they are defined (measured:
// with the step kernels and the queue in separate modules the queue's diagonal factorisation came out with different address
// arithmetic).  tools/isa_diff.py compares the device assembly of two builds symbol by symbol; a refactor of these files should
// leave it without a difference.  Host-only code lives in chol_tasklist.hip (plain C++, where every environment switch is read).
#include <mutex>
#include <vector>
#include "gp_device.hpp"
#include "chol_tiles.hpp"
#include "chol_steps.hpp"
#include "chol_queue.hpp"
#include "chol_prof.hpp"

namespace alabi {

static int tiles_in_cols(int ntr, int tc0, int tc1) {
    int n = 0;
    for (int tj = tc0; tj < tc1; ++tj) n += ntr - tj;
    return n;
}

// The list on the device, built once per (device, nb, list-shaping switches) and kept.
static int chol_task_list(int nb, const CholListShape& sh, const CholTask** dev, int* count) {
    struct Entry { int device, nb; CholListShape sh; CholTask* tasks; int count; };
    static std::mutex mu;
    static std::vector<Entry> cache;
    int device = 0;
    ALABI_HIP_CHECK(hipGetDevice(&device));
    std::lock_guard<std::mutex> lk(mu);
    for (const Entry& e : cache)
        if (e.device == device && e.nb == nb && e.sh == sh) { *dev = e.tasks; *count = e.count; return ALABI_OK; }
    std::vector<CholTask> t;
    chol_single_tasks(nb, sh, t);
    CholTask* d = nullptr;
    ALABI_HIP_CHECK(hipMalloc(&d, t.size() * sizeof(CholTask)));
    ALABI_HIP_CHECK(hipMemcpy(d, t.data(), t.size() * sizeof(CholTask), hipMemcpyHostToDevice));
    cache.push_back({device, nb, sh, d, (int)t.size()});
    *dev = d; *count = (int)t.size();
    return ALABI_OK;
}

// Will the task queue factorise this matrix?  If so its control words exist and *ctl_ints says how many the assembly kernel
// has to clear (queue head, time-out flag, tile versions, slab counters).
int cholesky_tasks_prepare(alabi_gp* gp, hipStream_t s, int* ctl_ints_out) {
    *ctl_ints_out = 0;
    const int nb = gp->Npad / 64;
    // Default for 3..256 block columns (N = 129..16384; ALABI_CHOL_TASKS=0 forces it off).  With the eight-wave
    // kernel of round 3 (from 40 block columns on): N = 5000 1.79 ms, 8192 5.08, 10000 8.5 (39.2 TFLOP/s), 11000 10.9 (panels of 8:
    // 12.6), 12000 13.6 (15.4), 14000 20.6 (22.9), 16000 29.7 (30.6) -- profiles/r03_cholesky_w8_vs_w4.txt.  Before that: measured
    // (tools/prof_chol_tasks.py, assembly included; round 3, updates over groups of block columns): N = 1024 0.33 ms (0.46 launch
    // per step), 2000 0.59 (0.89), 3072 0.96 (1.39), 4096 1.40 (2.05), 5000 2.0 (2.9), 6000 2.86 (3.96), 8192 5.9 (6.9),
    // 10000 9.9 (10.8 panels of 8), 12000 15.9 (15.4), 16000 35.1 (30.5): from 11000 on the rank-512 panel path is ahead.
    const CholSwitches sw = chol_switches();
    const bool forced_on = chol_queue_forced_on(sw), forced_off = chol_queue_forced_off(sw);
    // From 3 block columns on since the end of round 4 (tools/prof_chol_small.py, queue vs launch per step: N = 192 0.092 vs 0.112 ms, 512 0.155 vs
    // 0.230, 960 0.249 vs 0.408 -- with the matrix-core panel solves the queue wins at every size; before, it started at 16 block columns).
    if (nb < 3 || nb > 256 || forced_off || (!forced_on && nb > ALABI_CHOL_TASKS_MAX_NB)) return ALABI_OK;
    const size_t ctl_ints = 2 + (size_t)nb * nb + nb + 130;            // + 130: alignment + phase timers of an ALABI_CHOL_PROF build
    // behind the control words (8-byte aligned; filled with the tag by the assembly kernel): the slab buffers, [nb][4][64][16] doubles
    auto total_ints = [](size_t b) { return ((2 + b * b + b + 130 + 1) & ~(size_t)1) + b * 8192; };
    if (gp->chol_ctl_ints < total_ints(nb)) {
        if (gp->chol_ctl) { ALABI_HIP_CHECK(hipStreamSynchronize(s)); ALABI_HIP_CHECK(hipFree(gp->chol_ctl)); gp->chol_ctl = nullptr; }
        const size_t cap_nb = gp->n_cap / 64 < 256 ? gp->n_cap / 64 : 256;
        const size_t cap = total_ints(cap_nb), need = total_ints(nb);
        ALABI_HIP_CHECK(hipMalloc(&gp->chol_ctl, (cap > need ? cap : need) * sizeof(int)));
        gp->chol_ctl_ints = cap > need ? cap : need;
    }
    *ctl_ints_out = (int)ctl_ints;
    return ALABI_OK;
}

// 1 when the queue kernel was launched (the caller reads gp->chol_ctl[1] after its synchronisation: non-zero = a wait ran out,
// the matrix is in an undefined state and must be assembled and factorised again on the launch-per-step path).  The control
// words and gp->info were cleared by launch_assemble(gp, s, ctl_ints).
int launch_cholesky_tasks(alabi_gp* gp, hipStream_t s, int* launched) {
    *launched = 0;
    const int ld = gp->Npad, nb = gp->Npad / 64;
    const CholTask* tasks = nullptr;
    int ntasks = 0, st;
    const CholSwitches sw = chol_switches();
    if ((st = chol_task_list(nb, sw.list, &tasks, &ntasks)) != ALABI_OK) return st;
    const int n_cu = device_cu_count();
    int grid = ntasks < n_cu ? ntasks : n_cu;
    const int spin = sw.spin_limit;
    // eight waves per workgroup from ALABI_CHOL_W8_MIN_NB block columns on (ALABI_CHOL_W8=0 / 1 forces four / eight)
    const bool w8 = chol_tasks_w8(nb, sw.list);
    if (w8) hipLaunchKernelGGL(chol_tasks8_kernel, dim3(grid), dim3(512), 0, s, gp->L, ld, nb, tasks, ntasks, gp->chol_ctl, gp->info, gp->dinv, spin);
    else hipLaunchKernelGGL(chol_tasks_kernel, dim3(grid), dim3(256), 0, s, gp->L, ld, nb, tasks, ntasks, gp->chol_ctl, gp->info, gp->dinv, spin);
    ALABI_LAUNCH_CHECK();
    chol_report_instrumentation(gp, nb, sw, s);
    *launched = 1;
    return ALABI_OK;
}

// The launch-per-step factorisation of ONE [Npad, Npad] matrix (any owner: a GP handle, a slot of a batch workspace).
int launch_cholesky_steps(double* L, int Npad, int* info, double* dinv, hipStream_t s) {
    const int ld = Npad, nb = Npad / 64;
    // (info was cleared by the assembly kernel, which always runs just before)
    hipLaunchKernelGGL(potrf_diag_kernel, dim3(1), dim3(64), 0, s, L, ld, 0, info, dinv);
    // Block columns per panel (0: rank-64 updates of the whole trailing matrix).  Measured on MI355X (tools/prof_cholesky.py):
    // the panel path wins from about N = 8000 on (N = 10000: 14.3 -> 11.3 ms, N = 16000: 49.6 -> 31.4 ms with panels of 8;
    // panels of 4: 11.8 / 33.0 ms); below that the extra launches per panel cost more than the trailing traffic they save
    // (N = 5000: 3.2 vs 3.9 ms).
    const CholSwitches sw = chol_switches();
    const int panel = sw.panel != CHOL_UNSET ? sw.panel : nb >= 110 ? 8 : 0;                          // N >= 7040 (N = 7000: 5.33 vs 5.54 ms rank-64, 7500: 6.05 vs 6.59; 6500: 4.80 vs 4.73)
    if (panel == 0) {
        for (int kb = 0; kb + 1 < nb; ++kb) {
            const int T = nb - kb - 1;
            hipLaunchKernelGGL(trsm_panel_kernel, dim3(T), dim3(256), 0, s, L, ld, kb, dinv);
            hipLaunchKernelGGL(syrk_update_kernel, dim3(T * (T + 1) / 2), dim3(256), 0, s, L, ld, kb, info, dinv, 0, T);   // + potrf of block kb+1
        }
        ALABI_LAUNCH_CHECK();
        return ALABI_OK;
    }
    // Panels of `panel` block columns.  Inside a panel: trsm of block column kb, rank-64 update of the REST OF THE PANEL only
    // (with the factorisation of the next diagonal block fused in).  Behind it: one rank-(64 panel) update of the trailing
    // matrix, split for look-ahead -- the tile columns of the next panel on the caller's stream (the next panel's chain of
    // small launches waits only for them), everything further right on a second stream, overlapping that chain.
    // (per host thread: the cross-validation search factorises on several threads and streams at once)
    static thread_local hipStream_t side = nullptr;
    static thread_local hipEvent_t ev_panel[2] = {nullptr, nullptr}, ev_rest[2] = {nullptr, nullptr};
    const bool lookahead = chol_lookahead(sw);
    if (lookahead && !side) {
        // lowest priority: the bulk update fills every CU (two workgroups each); whenever one of them retires, the waiting
        // workgroups of the next panel's chain on the caller's stream are dispatched first
        int prio_least = 0, prio_greatest = 0;
        ALABI_HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
        ALABI_HIP_CHECK(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, prio_least));
        for (int i = 0; i < 2; ++i) {
            ALABI_HIP_CHECK(hipEventCreateWithFlags(&ev_panel[i], hipEventDisableTiming));
            ALABI_HIP_CHECK(hipEventCreateWithFlags(&ev_rest[i], hipEventDisableTiming));
        }
    }
    bool rest_pending = false;
    int pi = 0;
    for (int p0 = 0; p0 < nb; p0 += panel, ++pi) {
        const int pe = p0 + panel < nb ? p0 + panel : nb;
        for (int kb = p0; kb < pe; ++kb) {
            const int T = nb - kb - 1;
            if (T == 0) break;
            hipLaunchKernelGGL(trsm_panel_kernel, dim3(T), dim3(256), 0, s, L, ld, kb, dinv);
            const int jc = pe - kb - 1;
            if (jc > 0) {
                int tiles = 0;
                for (int tj = 0; tj < jc; ++tj) tiles += T - tj;
                hipLaunchKernelGGL(syrk_update_kernel, dim3(tiles), dim3(256), 0, s, L, ld, kb, info, dinv, jc, T);
            }
        }
        if (pe >= nb) break;
        const int row0 = 64 * pe, ntr = (Npad - row0 + 127) / 128, kp = 64 * (pe - p0);
        const int next_tc = (panel * 64) / 128;          // tile columns that make up the next panel
        const int tc_split = next_tc < ntr ? next_tc : ntr;
        if (lookahead) {
            // the rest of the PREVIOUS panel's update touched the tiles we are about to update: wait for it
            if (rest_pending) ALABI_HIP_CHECK(hipStreamWaitEvent(s, ev_rest[(pi + 1) & 1], 0));
            ALABI_HIP_CHECK(hipEventRecord(ev_panel[pi & 1], s));                       // panel pi is final
            hipLaunchKernelGGL(syrk_panel_kernel<true>, dim3(tiles_in_cols(ntr, 0, tc_split)), dim3(256), 0, s, L, ld, Npad, 64 * p0, kp,
                               row0, 0, tc_split, ntr, info, dinv);
            if (tc_split < ntr) {
                ALABI_HIP_CHECK(hipStreamWaitEvent(side, ev_panel[pi & 1], 0));
                hipLaunchKernelGGL(syrk_panel_kernel<false>, dim3(tiles_in_cols(ntr, tc_split, ntr)), dim3(256), 0, side, L, ld, Npad,
                                   64 * p0, kp, row0, tc_split, ntr, ntr, info, (double*)nullptr);
                ALABI_HIP_CHECK(hipEventRecord(ev_rest[pi & 1], side));
                rest_pending = true;
            } else {
                rest_pending = false;
            }
        } else {
            hipLaunchKernelGGL(syrk_panel_kernel<true>, dim3(tiles_in_cols(ntr, 0, ntr)), dim3(256), 0, s, L, ld, Npad, 64 * p0, kp, row0,
                               0, ntr, ntr, info, dinv);
        }
    }
    if (lookahead && rest_pending) ALABI_HIP_CHECK(hipStreamWaitEvent(s, ev_rest[(pi + 1) & 1], 0));
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

int launch_cholesky(alabi_gp* gp, hipStream_t s) { return launch_cholesky_steps(gp->L, gp->Npad, gp->info, gp->dinv, s); }
// ---------------------------------------------------------------------------------------------------------------------
// Batched task queue: B independent matrices in ONE launch of chol_tasks8_batch_kernel (gp_batch.hip is the caller; how the
// matrices' lists are interleaved: chol_batch_build in chol_tasklist.hip).
void chol_batch_free(CholBatchQueue& q) {
    if (q.tasks) (void)hipFree(q.tasks);
    if (q.list_off) (void)hipFree(q.list_off);
    if (q.mats) (void)hipFree(q.mats);
    if (q.ctl) (void)hipFree(q.ctl);
    if (q.linv) (void)hipFree(q.linv);
    q = CholBatchQueue{};
}

// Queue B matrices (slot b: A[b] [ld[b], ld[b]] row-major with ld a multiple of 64, dinv[b] [ld[b]], info[b] [1], all device memory):
// builds (or reuses) the interleaved task list, uploads the matrix table, clears the control words -- everything on `s`.
int chol_batch_prepare(CholBatchQueue& q, int B, const int* ld, double* const* A, double* const* dinv, int* const* info, hipStream_t s) {
    if (B <= 0 || B >= 32768) return ALABI_BAD_ARGUMENT;
    const CholSwitches sw = chol_switches();
    int nlists = sw.batch_lists, window = sw.batch_window;   // defaults 8, 8; measured: window 2 45 ms, 3 40, 4 35.6, 5 33.2, 8 31.8, 0 (all at once) 31.4-32.4 per 500 matrices of N = 1600
    if (nlists > B) nlists = B;
    while (nlists > 1 && B < 4 * nlists && B % nlists != 0) nlists /= 2;   // few (large) matrices: equal shares per list (12 matrices of N = 8000: 8 lists 5.7 ms per fit, 4 lists 5.2)
    std::vector<int> nbs(B);
    size_t ver_ints = 0;
    for (int b = 0; b < B; ++b) {
        if (ld[b] <= 0 || ld[b] % 64 != 0 || ld[b] / 64 > 256) return ALABI_BAD_ARGUMENT;
        nbs[b] = ld[b] / 64;
        ver_ints += (size_t)nbs[b] * nbs[b] + nbs[b];
    }
    if (!(q.tasks && q.nbs == nbs && q.nlists == nlists && q.window == window && q.shape == sw.list)) {
        std::vector<CholTask> t;
        std::vector<int> lo;
        chol_batch_build(nbs, nlists, window, sw.list, t, lo);
        if (t.size() > q.tasks_cap) {
            if (q.tasks) { ALABI_HIP_CHECK(hipStreamSynchronize(s)); (void)hipFree(q.tasks); q.tasks = nullptr; q.tasks_cap = 0; }
            ALABI_HIP_CHECK(hipMalloc(&q.tasks, t.size() * sizeof(CholTask)));
            q.tasks_cap = t.size();
        }
        if (!q.list_off) ALABI_HIP_CHECK(hipMalloc(&q.list_off, 9 * sizeof(int)));
        ALABI_HIP_CHECK(hipStreamSynchronize(s));                         // a launch still reading the previous list
        ALABI_HIP_CHECK(hipMemcpy(q.tasks, t.data(), t.size() * sizeof(CholTask), hipMemcpyHostToDevice));
        ALABI_HIP_CHECK(hipMemcpy(q.list_off, lo.data(), (nlists + 1) * sizeof(int), hipMemcpyHostToDevice));
        q.ntasks = (int)t.size(); q.nbs = nbs; q.nlists = nlists; q.window = window; q.shape = sw.list;
    }
    if ((size_t)B > q.mats_cap) {
        if (q.mats) { ALABI_HIP_CHECK(hipStreamSynchronize(s)); (void)hipFree(q.mats); q.mats = nullptr; }
        ALABI_HIP_CHECK(hipMalloc(&q.mats, (size_t)B * sizeof(CholMat)));
        q.mats_cap = B;
    }
    const size_t ctl_ints = 256 + ver_ints;
    if (ctl_ints > q.ctl_cap) {
        if (q.ctl) { ALABI_HIP_CHECK(hipStreamSynchronize(s)); (void)hipFree(q.ctl); q.ctl = nullptr; }
        ALABI_HIP_CHECK(hipMalloc(&q.ctl, ctl_ints * sizeof(int)));
        q.ctl_cap = ctl_ints;
    }
    q.ctl_ints = ctl_ints;
    size_t linv_doubles = 0;                                              // the slab buffers, [nb][4][64][16] per matrix (not cleared: the batch polls the slab counters)
    for (int b = 0; b < B; ++b) linv_doubles += (size_t)nbs[b] * 4096;
    if (linv_doubles > q.linv_cap) {
        if (q.linv) { ALABI_HIP_CHECK(hipStreamSynchronize(s)); (void)hipFree(q.linv); q.linv = nullptr; }
        ALABI_HIP_CHECK(hipMalloc(&q.linv, linv_doubles * sizeof(double)));
        q.linv_cap = linv_doubles;
    }
    std::vector<CholMat> hm(B);
    size_t off = 256, loff = 0;
    for (int b = 0; b < B; ++b) {
        hm[b].A = A[b]; hm[b].dinv = dinv[b]; hm[b].info = info[b]; hm[b].ld = ld[b]; hm[b].nb = nbs[b];
        hm[b].ver = q.ctl + off; hm[b].sver = q.ctl + off + (size_t)nbs[b] * nbs[b];
        hm[b].linv = q.linv + loff;
        off += (size_t)nbs[b] * nbs[b] + nbs[b];
        loff += (size_t)nbs[b] * 4096;
    }
    ALABI_HIP_CHECK(hipMemcpyAsync(q.mats, hm.data(), (size_t)B * sizeof(CholMat), hipMemcpyHostToDevice, s));
    ALABI_HIP_CHECK(hipStreamSynchronize(s));                             // `hm` is a local
    ALABI_HIP_CHECK(hipMemsetAsync(q.ctl, 0, ctl_ints * sizeof(int), s));
    q.B = B;
    return ALABI_OK;
}

// One launch of the batched queue; the time-out flag is q.ctl[1] (read it after synchronising: non-zero = undefined matrices).
int chol_batch_launch(CholBatchQueue& q, hipStream_t s) {
    const int n_cu = device_cu_count();
    const int grid = q.ntasks < n_cu ? q.ntasks : n_cu;
    const int spin = chol_switches().spin_limit;
    hipLaunchKernelGGL(chol_tasks8_batch_kernel, dim3(grid), dim3(512), 0, s, q.mats, q.tasks, q.ntasks, q.list_off, q.nlists, q.ctl, spin);
    ALABI_LAUNCH_CHECK();
    return ALABI_OK;
}

}  // namespace alabi

