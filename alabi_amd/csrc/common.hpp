// Shared declarations for libalabi_hip.so (gfx950 / MI355X only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/alabi_hip.h"
#include "chol_tasks.hpp"
#include "predict_plan.hpp"
#include "ens_plan.hpp"

#define ALABI_BLK 64  // Cholesky / TRSM block edge; matrices are padded to a multiple of it

namespace alabi {

extern thread_local std::string g_last_error;

inline int hip_fail(hipError_t e, const char* what, const char* file, int line) {
    char buf[512];
    snprintf(buf, sizeof(buf), "%s failed at %s:%d: %s", what, file, line, hipGetErrorString(e));
    g_last_error = buf;
    return ALABI_HIP_ERROR;
}

#define ALABI_HIP_CHECK(expr)                                                    \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess) return ::alabi::hip_fail(_e, #expr, __FILE__, __LINE__); \
    } while (0)

#define ALABI_LAUNCH_CHECK() ALABI_HIP_CHECK(hipGetLastError())

// Per-dimension scale passed by value to kernels (kernel-argument space, graph safe).
struct DimVec {
    double v[ALABI_MAX_DIM];
};

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// CUs of the current device; 256 when the query fails
inline int device_cu_count() {
    int dev = 0, n_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n_cu <= 0) n_cu = 256;
    return n_cu;
}

// Radial part of the stationary kernel: k(x,x') = amp * f(r2), r2 = sum_k (x_k - x'_k)^2 / M_k.
//   0 ExpSquaredKernel exp(-r2/2)              1 Matern32Kernel (1 + s) exp(-s), s = sqrt(3 r2)
//   2 Matern52Kernel (1 + s + s^2/3) exp(-s), s = sqrt(5 r2)     3 RationalQuadraticKernel (1 + r2/(2a))^-a
// (george kernel definitions; reference: alabi/core.py:1000-1014)
struct KernelFn {
    int type;
    double alpha;
};

}  // namespace alabi

// ---- handle layouts ------------------------------------------------------------------
struct alabi_gp {
    int n_cap = 0;     // capacity in training points (multiple of ALABI_BLK)
    int d = 0;
    int N = 0;         // current number of training points
    int Npad = 0;      // N rounded up to ALABI_BLK; leading dimension of L and Xt rows
    bool computed = false;
    bool has_alpha = false;
    long long gen = 0;  // bumped by every compute / set_y / set_hyper
    int last_pivot = 0;
    int factor_path = 0;      // alabi_gp_last_factor_path
    double* point_host = nullptr;   // alabi_gp_predict_grad_point: pinned [3 + 3 d] (the point, then mu, var, dmu, dvar)
    double* point_dev = nullptr;    // the same on the device
    // hyper-parameters (host copies)
    double mean = 0.0, log_wn = -12.0, log_amp = 0.0;
    alabi::KernelFn kf{0, 1.0};   // kernel family (+ alpha of the rational quadratic)
    double log_M[ALABI_MAX_DIM];
    alabi::DimVec inv_len;  // exp(-0.5 log_M): coordinates are pre-multiplied by it
    // device buffers
    double* L = nullptr;      // [n_cap, n_cap] row-major, lower triangle holds chol(K)
    double* Xt = nullptr;     // [d, n_cap]  scaled, transposed training inputs (SoA)
    double* Xa = nullptr;     // [round_up(d + 2, 4), n_cap] augmented rows (Xt, -|x|^2 / 2, 1, 0..) for the matrix-core predict-mean kernel
    long long xa_gen = -1;    // factor_gen the rows belong to (built lazily)
    double* xa_centre = nullptr;   // [ALABI_MAX_DIM] mean of the scaled training inputs: Xa rows and the query operands are taken relative to it
    double* y = nullptr;      // [n_cap]
    double* alpha = nullptr;  // [n_cap]
    double* dinv = nullptr;   // [n_cap] 1 / L_ii (every triangular solve multiplies by it)
    double* work = nullptr;   // [2 * n_cap] solve scratch
    double* work2 = nullptr;  // [n_cap] hand-off buffer of the dataflow solve
    int* flags = nullptr;     // [1] time-out flag of the dataflow solve
    double* red = nullptr;    // [4] reductions (logdet, r.alpha)
    int* info = nullptr;      // [1] Cholesky info (0 ok, else 1-based pivot)
    int* host_status = nullptr;   // pinned [2]: read-back of (info, task-queue time-out) after a factorisation
    int* chol_ctl = nullptr;  // task-queue factorisation: [0] queue head, [1] time-out flag, [2 + i * nb + j] tile versions
    size_t chol_ctl_ints = 0;
    double* ws = nullptr;     // predict-variance workspace
    size_t ws_bytes = 0;
    double* scan = nullptr;   // utility-scan scratch (partials)
    size_t scan_bytes = 0;
    double* winv = nullptr;   // L^-1, tile-major: every variance request, the gradients and the append step multiply with it (built lazily per factor)
    size_t winv_bytes = 0;
    long long factor_gen = 0; // bumped by every successful compute
    long long winv_gen = -1;  // factor_gen the cached L^-1 belongs to
    double* small = nullptr;  // [Npad / 64][16] partial sums of the small-batch variance kernel
    size_t small_bytes = 0;
    double* mupart = nullptr; // partial mean sums of the K* pre-pass when the training points are split over workgroups
    size_t mupart_bytes = 0;
    double* pgrad = nullptr;  // scratch of the query-gradient path (v, |v|^2 partials, z parts)
    size_t pgrad_bytes = 0;
    // ensemble kernels, squared exponential (ens_device.hpp: se_pair_terms): the scaled training inputs relative to their mean
    // (xa_centre) and h_n = |x_n - c|^2 / 2 - ln|alpha_n| with sign(alpha_n) in the lowest mantissa bit, rebuilt whenever `gen` moves
    double* Xc = nullptr;     // [dim_bucket(d), Npad]
    double* ens_h = nullptr;  // [Npad]
    long long ens_h_gen = -1;
    int solve_path = 0;       // alabi_gp_last_solve_path: which kernels produced alpha (launch_alpha)
};

namespace alabi {
// Per-chunk draw buffers, all [chunk_cap, E, W]; the first five are the proposal records in LIST order
// (per ensemble: set 0 then set 1), the last three keep the raw draws for export / tests.
struct DrawBuffers {
    int* order;      // global walker id at each list position
    int* cw;         // global id of the partner walker drawn for that position
    double* zz;      // stretch factor z (differential-evolution record: the step size gamma)
    double* lnfac;   // (d-1) ln z (differential-evolution record: 0)
    double* lnu;     // ln u'
    int* partner;    // raw partner index into the complementary list (by list position)
    double* u_z;     // raw uniforms (by list position)
    double* u_acc;
    unsigned long long* packed;   // 4 words per list position: walker | partner << 32, zz, lnfac, lnu (persistent kernel)
    int* pos_of;     // list position (0..W-1 within the ensemble) of every walker, keyed by global walker id (inverse of `order`)
    unsigned long long* link;     // group kernel: 2 words per list position, where the two rows the proposal reads were produced (ens_link_kernel)
    unsigned long long* packed_x; // pair kernel with placement: `packed`, every half step permuted so that position = pair (ens_place_kernel);
    int* place;                   // ... and the pair of every item, by list position.  Both allocated on first use.
};

// Proposal moves (emcee's `moves=`): one move per step and ensemble, chosen by ens_draw_kernel from cumulative weights.
//   kind 0 StretchMove: p0 = a.   kind 1 DEMove: p0 = gamma0 (mean step), p1 = sigma (its relative scatter).
//   kind 2 SnookerMove: p0 = gammas (the fixed step along the line), p1 = 0.
//   kind 3 WalkMove: p0 = s0, the size of the subset of the complementary half (0: all of it), p1 = 0.
//   kind 4 KDEMove: p0 / p1 = the bandwidth factor f of split 0 / split 1 (the two halves of an odd W differ in size).
//   kind 5 GaussianMove: p0 = ln factor (0: no scale factor), p1 = mode (0 vector, 1 random, 2 sequential); the scale factor C of
//   the proposal q = x + f C z travels apart from the table, ahead of it (alabi_ens_set_move_scale).
// n = 0 stands for the default, one stretch move with the `a` of the call.
#define ALABI_MAX_MOVES 8
struct MoveTable {
    int n;
    int kind[ALABI_MAX_MOVES];
    double cum[ALABI_MAX_MOVES];   // np.cumsum(w / w.sum()), formed on the host
    double p0[ALABI_MAX_MOVES], p1[ALABI_MAX_MOVES];
};
// What a differential-evolution record carries beyond DrawBuffers (kept apart from it: the persistent kernels take DrawBuffers by
// value and know one partner only).  A DE record reuses the stretch record's slots -- cw = C[j1], zz = gamma, lnfac = 0 -- and adds
// the second partner.  Allocated when a move set is given (alabi_ens_set_moves); null pointers are not written.
// A snooker record (ter Braak & Vrugt 2008) names three walkers of the complementary set: cw = z = C[j1], cw2 = z1 = C[j2] and the
// third partner z2 = C[j3]; zz = gammas, and lnfac is a placeholder (0): the factor depends on the rows and is formed by the kernel
// that forms the proposal.  The third-partner arrays exist only on a handle that was given a snooker move.
struct MoveBuffers {
    int* cw2;        // [chunk_cap, E, W] global id of the second partner C[j2] by list position; -1: a stretch record
    int* partner2;   // [chunk_cap, E, W] raw j2 into the complementary list (-1: stretch), for export / tests
    int* move;       // [chunk_cap, E] index of the step's move
    int* cw3;        // [chunk_cap, E, W] global id of the third partner C[j3]; -1: a stretch or differential-evolution record
    int* partner3;   // [chunk_cap, E, W] raw j3 into the complementary list (-1: stretch, DE), for export / tests
    // walk and KDE moves (kinds 3, 4): their proposals read the whole complementary half, so a record names no partner; the
    // half-step kernel takes the kind and the parameters of the step's move from here.  Allocated with the third-partner arrays
    // on a handle that was given such a move.
    int* kind;       // [chunk_cap, E] kind of the step's move
    double* par;     // [chunk_cap, E, 2] its p0, p1
};
// What ens_kde_prepass_kernel leaves for the KDE proposals of ONE half step (per ensemble): rewritten in front of every half step
// whose move is a KDE move.  Lives in HBM / L2: Nc x d doubles do not fit the LDS at Nc = 1024, d = 64.
struct KdeBuffers {
    double* white;   // [E, ncmax, d] the whitened rows L^-1 (c_j - mean) of the complementary half
    double* L;       // [E, d, d] lower Cholesky factor of H = f^2 cov (row-major; the upper triangle is not written)
    double* mean;    // [E, d] mean of the complementary half
    int* flag;       // [E] 1: a pivot of the factorisation was not positive and finite, every proposal of the half step is rejected
    unsigned long long* singular;   // [1] half steps (per ensemble) that were rejected so
};
// Draws of the walk and KDE test entries (alabi_ens_step_with_randoms_walk / _kde), keyed by WALKER id; null: counter-based draws.
struct WkInject {
    const int* idx;      // walk: [W, s0] subset indices into the complementary list; KDE: [W] the row r
    const double* z;     // walk: [W, s0] the normals of the subset's rows; KDE: [W, d]
    double* lnfac_out;   // KDE: [W] the proposals' log factor, by walker id (nullable)
};
}  // namespace alabi

struct alabi_ens {
    alabi_gp* gp = nullptr;
    int W = 0, d = 0, E = 1;
    int n_cu = 0;             // CUs of the device the handle was created on (device_cu_count), read by every rule of ens_plan.hip
    int threads = 1024;       // workgroup size of the half-step kernel
    double lp_scale = 1.0, lp_shift = 0.0;   // log-probability = lp_scale * GP mean + lp_shift inside the box (y scaler)
    // independent normal priors on selected coordinates (lnprior_normal): mean, 1 / std (0 = none), sum of the constants
    double prior_mean[ALABI_MAX_DIM] = {0}, prior_istd[ALABI_MAX_DIM] = {0};
    double prior_const = 0.0;
    int has_prior = 0;
    int ymap = 0;             // inverse y scaler applied to the GP mean inside the kernels (0 identity, 1 -10^x, 2 10^x)
    unsigned long long seed = 0;
    double lo[ALABI_MAX_DIM], hi[ALABI_MAX_DIM];
    double* consts = nullptr; // device [3][ALABI_MAX_DIM]: inv_len, lo, hi
    long long consts_gen = -1;
    int chunk_cap = 0;        // steps the draw buffers hold
    int drawn_n = 0;
    alabi::DrawBuffers draws{};
    // graph cache for the single-GPU run loop
    hipGraphExec_t graph_exec = nullptr;
    struct GraphKey {
        void *coords, *logp, *chain, *chain_logp, *n_accept;
        int thin_by, nsteps;
        double a;
        long long gp_gen;  // generation counter of the GP (re-capture after a refit)
    } graph_key{};
    int graph_steps = 0;
    long long* run_state = nullptr;  // device [4]: [0] first global step of the chunk, [1] steps done before it
    // persistent dataflow path (ens_stream_kernel)
    unsigned long long* hist = nullptr;  // [(chunk_cap+1)][E*W][d+1] version history of every walker
    int* err = nullptr;                  // [1] spin time-out flag: the first word of state_dev
    // What a stream call reads back, one copy: [err (one 8-byte word) | coords [E*W, d] | logp [E*W]] on the device (the last chunk's
    // epilogue writes the walkers there) and the same layout in pinned host memory (alabi_ens_last_state copies from it)
    unsigned long long* state_dev = nullptr;
    unsigned long long* state_host = nullptr;
    bool last_state_ok = false;          // state_host holds the walkers the last alabi_ens_run left (it ended cleanly on ens_stream_kernel / ens_pair_kernel)
    // (coords, logp, n_accept) at the start of a persistent call (ens_call_prologue_kernel): a time-out of the pair variant is retried
    // on ens_stream_kernel from here, and alabi_ens_restore hands it back to a caller who repeats the call on another path
    double* save = nullptr;
    bool save_valid = false, save_accept = false;       // a save was taken; it holds the acceptance counters too
    // draws one chunk ahead: second set of draw buffers, filled on a library-owned side stream while the previous chunk's persistent
    // kernel runs, and at the end of a call for the first chunk of the next (allocated on first use; draws2_state -1: not available,
    // single buffer, every draw on the main stream)
    alabi::DrawBuffers draws2{};
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_free = nullptr, ev_drawn = nullptr;   // main -> side: the buffer is no longer read; side -> main: the draws are there
    int draws2_state = 0;
    int draw_set = 0;                    // the set the next chunk's records come from: 0 draws, 1 draws2
    // the records draws2 holds for a call that has not come yet (drawn behind the last persistent kernel of the previous one): valid for
    // a call that starts at ahead_step with the same `a` and move table and takes at most ahead_n steps in its first chunk
    bool ahead_valid = false, ahead_pending = false;    // pending: ev_drawn stands for a launch on the side stream nobody has waited for
    long long ahead_step = 0, ahead_moves_gen = 0;
    double ahead_a = 0.0;
    int ahead_n = 0;
    long long moves_gen = 0;             // bumped by alabi_ens_set_moves
    long long boundary_stats[4] = {0, 0, 0, 0};         // alabi_ens_boundary_stats: draw-ahead hits, misses, prop fills, hist fills launched
    int hist_clean = 0;                  // rows 1..hist_clean hold the sentinel (left so by ens_hist_epilogue_kernel); rows beyond are filled before use
    int prop_clean = 0;                  // the same for prop, whose words the epilogue of a pair chunk resets beside those of hist
    int stream_grid = 0;                 // workgroups per ensemble of the persistent kernel
    int last_path = 0;                   // route of the last alabi_ens_run (ens_plan.hpp: EnsRoute): 0 one launch per half step, 1 persistent kernel
                                         // (ens_stream_kernel / ens_pair_kernel), 3 ens_group_kernel, 4 ens_mh_kernel, 5 ens_hmc_kernel, 6 ens_nuts_kernel
    int stream_ok = 0;                   // eligible: training set fits the lanes' registers, one workgroup per CU
    // pair variant of the persistent kernel (ens_pair_kernel)
    unsigned long long* prop = nullptr;  // [(chunk_cap+1)][E*W][d+2] published proposals, allocated on first use
#define ALABI_PAIR_STATS_WORDS 36
    unsigned long long* pair_stats = nullptr;   // [ALABI_PAIR_STATS_WORDS] debug counters: [0, 9) alabi_ens_pair_stats, [9, 15) alabi_ens_pair_stats2, [16, 36) alabi_ens_pair_stats3; allocated on request
    int pair_state = 0;                  // 0 undecided, 1 ready, -1 off (not eligible, ALABI_ENS_PAIR=0, or after a time-out of this handle)
    int last_variant = 0;                // persistent kernel of the last stream call: 0 ens_stream_kernel, 1 ens_pair_kernel
    // placement of the pair kernel's items by XCD class (ens_place.hip)
    int place_state = 0;                 // 0 undecided, 1 on, -1 off (n0 % 8 != 0, odd W, W > 256, ALABI_ENS_PLACE=0, no memory)
    unsigned long long* place_stats = nullptr;   // [2] items with a preferred class, items placed on it (every pre-pass of a run adds)
    bool ahead_placed = false;           // the records drawn ahead for the next call have been through ens_place_kernel
    // group kernel (ens_group_kernel: training set partitioned over the members of a group, proposals streamed through)
    unsigned long long* part = nullptr;  // [2 chunk_cap][E][NG][G][16 Q] partial kernel sums (allocated on first use)
    size_t part_words = 0;
    unsigned long long* cand = nullptr;  // [2 chunk_cap][E][n0][2 d + 4] candidate rows (proposal, old coordinates, logp, ln factors, prior)
    size_t cand_words = 0;
    long long settings_gen = 0;          // bumped by every setter that changes what captured launches carry (graph keys)
    long long serial = 0;                // unique per handle for the life of the process (a new handle at an old address is not the old one)
    int group_plan[8] = {0};  // blocking of the last group-kernel launch: Q, G, NG, RT, tpm, ltw, KS, LDS bytes (alabi_ens_group_plan)
    // proposal moves (alabi_ens_set_moves): the table the draw kernel chooses from, whether it holds a move that reads more than
    // one partner row -- has_de: a DE or a snooker move (then every run takes the launch-per-half-step path, whose kernels read the
    // second partner row), has_snooker: a snooker move (the three-partner instantiations) -- and the records' further-partner arrays
    alabi::MoveTable moves{};
    bool has_de = false, has_snooker = false;
    bool has_wk = false, has_kde = false;   // a walk or KDE move (the whole-half instantiations run); a KDE move (the pre-pass is launched)
    alabi::MoveBuffers mv{};
    alabi::KdeBuffers kde{};
    // Gaussian Metropolis moves (kind 5): the scale factors [ALABI_MAX_MOVES][d, d] on the device, one slot per move of the table;
    // gauss_staged: the slots alabi_ens_set_move_scale has filled since the last alabi_ens_set_moves, which accepts a Gaussian move
    // only on such a slot; gauss_diag: the slots whose factor is diagonal; all_gauss: every move of the table is a Gaussian move,
    // the set ens_mh_kernel runs (mh_ok: not turned off by alabi_ens_set_stream)
    double* gauss_C = nullptr;
    int gauss_staged = 0, gauss_diag = 0;
    bool has_gauss = false, all_gauss = false;
    int mh_ok = 1;
    int mh_plan[4] = {0};     // last ens_mh_kernel launch: threads, steps per launch, LDS bytes, tiled (alabi_ens_mh_plan)
    // HMC moves (kind 6): their scale factors share gauss_C / gauss_staged / gauss_diag with the Gaussian moves (a table holds one
    // kind or the other); all_hmc: every move of the table is an HMC move, the only table that holds one (ens_hmc_kernel runs it)
    bool all_hmc = false;
    int hmc_plan[4] = {0};    // last ens_hmc_kernel launch: threads, steps per launch, LDS bytes, tiled (alabi_ens_hmc_plan)
    // NUTS moves (kind 7): factors as kind 6; all_nuts: every move of the table is a NUTS move, the only table that holds one
    // (ens_nuts_kernel runs it).  The per-walker sums since the last reset (alabi_ens_nuts_stats), allocated with the first such table
    bool all_nuts = false;
    int nuts_plan[4] = {0};   // last ens_nuts_kernel launch: threads, transitions per launch, LDS bytes, tiled (alabi_ens_nuts_plan)
    long long* nuts_counts = nullptr;   // [E*W, 3] leaves, depths reached, divergent transitions
    double* nuts_accept = nullptr;      // [E*W] sum of the leaves' acceptance statistics
};

namespace alabi {
// gp_assemble.hip
int launch_prepare_inputs(alabi_gp* gp, const double* X, int N, hipStream_t s);
int launch_assemble(alabi_gp* gp, hipStream_t s, int zero_ctl_ints = 0);   // also clears gp->info and the first zero_ctl_ints words of gp->chol_ctl
int launch_kernel_matrix(const double* X1, int n1, const double* X2, int n2, int d, double amp,
                         const DimVec& inv_len, KernelFn kf, double* K, hipStream_t s);
// gp_cholesky.hip (launchers; device code in chol_tiles / chol_steps / chol_queue.hpp, task lists and switches in chol_tasklist.hip)
int launch_cholesky(alabi_gp* gp, hipStream_t s);
int cholesky_tasks_prepare(alabi_gp* gp, hipStream_t s, int* ctl_ints);   // > 0: the task queue will run, its control words (to be zeroed by the assembly)
int launch_cholesky_tasks(alabi_gp* gp, hipStream_t s, int* launched);
int launch_cholesky_steps(double* L, int Npad, int* info, double* dinv, hipStream_t s);   // launch-per-step path on a bare matrix
// batched task queue (gp_batch.hip): many independent matrices in one launch of chol_tasks8_batch_kernel
struct CholBatchQueue {
    std::vector<int> nbs;                       // key of the cached task list: block columns per matrix, lists, window, list-shaping switches
    int nlists = 0, window = 0, B = 0;
    CholListShape shape;
    CholTask* tasks = nullptr; size_t tasks_cap = 0; int ntasks = 0;
    int* list_off = nullptr;                    // device [nlists + 1]
    CholMat* mats = nullptr; size_t mats_cap = 0;
    int* ctl = nullptr; size_t ctl_ints = 0, ctl_cap = 0;   // [32 q] list heads, [1] time-out flag, from [256] on: per matrix tile versions + slab counters
    double* linv = nullptr; size_t linv_cap = 0;            // per matrix the slab buffers [nb][4][64][16] (chol_queue.hpp: what the panel solves read of a diagonal tile)
};
int chol_batch_prepare(CholBatchQueue& q, int B, const int* ld, double* const* A, double* const* dinv, int* const* info, hipStream_t s);
int chol_batch_launch(CholBatchQueue& q, hipStream_t s);
void chol_batch_free(CholBatchQueue& q);
// gp_solve.hip
int launch_alpha(alabi_gp* gp, hipStream_t s);
int launch_reductions(alabi_gp* gp, hipStream_t s);
// gp_predict.hip (launchers; device code in predict_mean / predict_var_subst / predict_var_winv.hpp, routes and switches in predict_plan.hip).
// The entry points of api.hip read predict_switches() once per call and hand it down.
int launch_predict_mean(alabi_gp* gp, const double* Xs, long long M, double* mu, const PredictSwitches& sw, hipStream_t s);
int ensure_xa(alabi_gp* gp, hipStream_t s);           // augmented, centred rows Xa of the current factor (matrix-core predict-mean, group ensemble kernel)
// Process-wide cache of the large scratch buffers (variance workspace, cached L^-1): the reference creates a new GP object
// for every refit (gp_utils.py:233), and a 1-2 GiB hipMalloc per new handle costs tens of milliseconds.
void* dev_cache_take(size_t need, size_t* bytes);   // a cached buffer of at least `need` bytes, or nullptr
void dev_cache_give(void* p, size_t bytes);         // hand a buffer back (may free it or another one)
int dev_alloc_cached(void** p, size_t need, size_t* bytes);   // cache first, then hipMalloc; hipError_t as int
// Grow-only scratch of a handle: afterwards *p holds at least `need` bytes.  A buffer that is too small is handed back first -- once
// the stream has drained, kernels in flight may still use it -- to the cache above (grow_cached: ws, winv) or to hipFree (grow_plain).
// grow_cached returns ALABI_NOT_COMPUTED when the memory cannot be had (*p is null then; the caller decides what that means),
// either returns ALABI_HIP_ERROR for a failed runtime call.
int grow_cached(double** p, size_t* bytes, size_t need, hipStream_t s);
int grow_plain(double** p, size_t* bytes, size_t need, hipStream_t s);
int launch_factor_inverse(alabi_gp* gp, hipStream_t s);
int launch_append(alabi_gp* gp, const double* x_new, hipStream_t s);   // gp_append.hip
int launch_factor_inverse_dnc(alabi_gp* gp, double* R, double* dst, hipStream_t s);   // gp_inverse.hip
int launch_predict_grad(alabi_gp* gp, const double* Xs, long long M, double* mu, double* var, double* dmu, double* dvar,
                        hipStream_t s);                                  // gp_predict_grad.hip
int ensure_winv(alabi_gp* gp, hipStream_t s);        // the cached L^-1 of the current factor in gp->winv (ALABI_NOT_COMPUTED: no room)
int launch_factor_inverse_into(alabi_gp* gp, double* dst, hipStream_t s);
int launch_predict_var_small(alabi_gp* gp, const double* Xs, int M, double* mu, double* var, const PredictSwitches& sw, hipStream_t s);
int launch_grad_log_likelihood(alabi_gp* gp, double* grad_dev, hipStream_t s);
int launch_get_inverse(alabi_gp* gp, double* Kinv_out, hipStream_t s);   // gp_grad.hip: K^-1 = W^T W, [N,N] row-major
int launch_predict_var(alabi_gp* gp, const double* Xs, long long M, double* mu, double* var, const PredictSwitches& sw,
                       hipStream_t s);
// utility.hip
int launch_utility_eval(int algo, const double* Xs, long long M, int d, const DimVec& lo,
                        const DimVec& hi, double y_best, const double* mu, const double* var,
                        double* u, hipStream_t s);
int launch_argmin(const double* u, long long M, double* partial_val, long long* partial_idx,
                  int nblocks, hipStream_t s);
// The shape of a handle for the rules of ens_plan.hip.  has_stream: the call was given a stream.
inline EnsShape ens_shape(const alabi_ens* e, bool has_stream = true) {
    EnsShape sh;
    sh.W = e->W; sh.E = e->E; sh.d = e->d; sh.Npad = e->gp->Npad;
    sh.generic = e->gp->kf.type != 0; sh.ymap = e->ymap;
    sh.threads = e->threads; sh.chunk_cap = e->chunk_cap; sh.stream_grid = e->stream_grid;
    sh.has_hist = e->hist && e->err;
    sh.stream_ok = e->stream_ok; sh.mh_ok = e->mh_ok;
    sh.has_de = e->has_de; sh.all_gauss = e->all_gauss; sh.all_hmc = e->all_hmc;
    sh.factors = e->gauss_C != nullptr;
    sh.n_moves = e->moves.n;
    for (int k = 0; k < e->moves.n; ++k) { const int L = hmc_leapfrog_of(e->moves.p1[k]); if (L > sh.lmax) sh.lmax = L; }
    sh.mh_lds = ens_mh_lds_bytes(e->moves.n, e->d);
    const size_t hl = ens_hmc_lds_bytes(e->moves.n, e->d, e->gp->Npad);
    sh.hmc_lds = hl > 0x7fffffffull ? 0x7fffffff : (int)hl;
    sh.has_stream = has_stream;
    sh.all_nuts = e->all_nuts;
    const size_t nl = ens_nuts_lds_bytes(e->moves.n, e->d, e->gp->Npad);
    sh.nuts_lds = nl > 0x7fffffffull ? 0x7fffffff : (int)nl;
    return sh;
}
// ensemble.hip.  The entry points of ens_api.hip / ens_run.hip / ens_sharded.hip read ens_switches() once per call and hand it
// down to the launchers that a switch concerns.
int ens_se_prepare(alabi_gp* gp, hipStream_t s);     // Xc and ens_h of the current (inputs, alpha) for the squared-exponential half-step kernels
struct HalfArgs {
    double* coords;              // [E*W,d] in/out
    double* logp;                // [E*W] in/out
    DrawBuffers rec;             // already offset to the step
    const double* consts;        // device [5][ALABI_MAX_DIM]: inv_len, lo, hi, prior mean, prior 1 / std
    const double* Xt;            // [D,Npad]
    const double* alpha;         // [Npad]
    const double* Xc;            // [D,Npad] the scaled inputs relative to their mean   } squared exponential, half-step kernels
    const double* ens_h;         // [Npad] |x - c|^2 / 2 - ln|alpha|, sign(alpha) in bit 0  } (se_pair_terms); see alabi_gp
    const double* centre;        // [d] mean of the scaled training inputs
    double* chain;               // [nstore,E*W,d] or null
    double* chain_logp;          // [nstore,E*W] or null
    long long* n_accept;         // [E*W] or null
    const long long* run_state;  // [0] chunk's first global step, [1] steps done before the chunk
    int n0, W, d, Npad, split, part_begin, local_t, thin_by;
    int count;                   // proposals in this launch (several per workgroup in ens_half_multi_kernel)
    int has_prior;               // consts rows 3 / 4 hold prior mean and 1 / std
    int ymap;                    // inverse y scaler on the GP mean: 0 identity, 1 -10^x (nlog_scaler), 2 10^x (log_scaler)
    double prior_const;
    double amp, mean;
    KernelFn kf;
    // sharded ensemble (ens_sharded.hip): the walker rows live in a history indexed by (half step, rank, slot); rec.link[2 pos] holds
    // the word offsets (own | partner << 32, -1 = the state in coords / logp) of the two rows a proposal reads, the result row
    // (coords, logp, accepted) of proposal blockIdx.x goes to sout + blockIdx.x (d + 2) and coords / logp are left alone
    const double* shist = nullptr;
    double* sout = nullptr;
    // differential-evolution records (MoveBuffers::cw2 offset to the step): set -> the kernels' two-partner instantiations run
    const int* cw2 = nullptr;
    // snooker records (MoveBuffers::cw3 offset to the step; cw2 is set as well): set -> the three-partner instantiations run
    const int* cw3 = nullptr;
    // walk and KDE steps (MoveBuffers::kind / ::par offset to the step; cw2 and cw3 are set as well): set -> the whole-half
    // instantiations run.  seed keys their counter-based draws, inj replaces them (test entries).
    const int* mvkind = nullptr;
    const double* mvpar = nullptr;
    KdeBuffers kde{};
    WkInject inj{};
    unsigned long long seed = 0;
    // Gaussian steps (kind 5): the index of the step's move (MoveBuffers::move offset to the step) and the moves' scale factors
    // [ALABI_MAX_MOVES][d, d] with bit k of gauss_diag set where factor k is diagonal.  Test entry: gauss_k >= 0 names the move,
    // gauss_f is the step's scale factor, inj.idx [W] the coordinate (-1: all), inj.z [W, d] the normals.
    const int* mvidx = nullptr;
    const double* gauss_C = nullptr;
    int gauss_diag = 0, gauss_k = -1;
    double gauss_f = 1.0;
};
int launch_ens_kde_prepass(alabi_ens* e, const HalfArgs& args, hipStream_t s);
int launch_ens_prep_wk(alabi_ens* e, const int* order, const double* u_acc, hipStream_t s);
int launch_ens_set_step_move(alabi_ens* e, int kind, double p0, double p1, hipStream_t s);
int launch_ens_gauss_export(alabi_ens* e, double* f, int* coord, double* z, hipStream_t s);   // the Gaussian draws of drawn step 0
int launch_ens_draw(alabi_ens* e, int nsteps, double a, hipStream_t s);
int launch_ens_draw_at(alabi_ens* e, const DrawBuffers& into, int nsteps, double a, bool from_state, long long step0, hipStream_t s);   // first step: run_state[0], or step0 by value
int launch_ens_prep(alabi_ens* e, const int* order, int n0, const double* u_z, const int* partner,
                    const double* u_acc, double a, hipStream_t s);
int launch_ens_prep_de(alabi_ens* e, const int* order, int n0, const int* j1, const int* j2, const double* gamma,
                       const double* u_acc, hipStream_t s);
int launch_ens_prep_snooker(alabi_ens* e, const int* order, int n0, const int* j1, const int* j2, const int* j3, double gamma,
                            const double* u_acc, hipStream_t s);
int launch_ens_half_args(alabi_ens* e, const HalfArgs& args, int nblocks, const EnsSwitches& sw, hipStream_t s);
// ens_mh.hip: all steps of a chunk of an all-Gaussian set in one launch, one workgroup per walker
int launch_ens_mh(alabi_ens* e, double* coords, double* logp, long long step0, long long done0, int K, int thin_by, double* chain,
                  double* chain_logp, long long* n_accept, hipStream_t s);
// ens_hmc.hip: all steps of a chunk of an all-HMC set in one launch, one workgroup per walker (inj_z: one step from injected draws)
int launch_ens_hmc(alabi_ens* e, double* coords, double* logp, long long step0, long long done0, int K, int thin_by, double* chain,
                   double* chain_logp, long long* n_accept, int inj_k, double inj_e, const double* inj_z, const double* inj_u, hipStream_t s);
int launch_ens_lp_grad(alabi_ens* e, const double* pts, int M, double* logp, double* grad, hipStream_t s);
// ens_hmc_adapt.hip: the same with a dual-averaged step size per walker (da_state [E*W, 5] in/out; par: delta, gamma, t0, kappa)
int launch_ens_hmc_adapt(alabi_ens* e, double* coords, double* logp, long long step0, long long done0, int K, int thin_by, double* chain,
                         double* chain_logp, long long* n_accept, double* da_state, const double* par, double* accept_stat, hipStream_t s);
// ens_map.hip: the multi-start BFGS ascent, the Hessian at arbitrary points, and the launch shape of the former
int launch_ens_map(alabi_ens* e, const double* starts, int S, int maxiter, double gtol, double* x_out, double* lp_out, int* iters_out,
                   int* status_out, double* gnorm_out, double* trace, int ntrace, hipStream_t s);
int launch_ens_lp_hess(alabi_ens* e, const double* pts, int M, double* hess, hipStream_t s);
void ens_map_plan(const alabi_ens* e, int* out);
int launch_ens_hmc_export(alabi_ens* e, long long step, int* move, double* e_out, double* z, double* u_acc, hipStream_t s);
// ens_nuts.hip: all transitions of a chunk of an all-NUTS set in one launch, one workgroup per walker (inj: one transition of move
// inj->k from injected draws, with its trace)
struct NutsInject {
    int k; double e;
    const double* z0; const unsigned* dir; const double* u_leaf; const double* u_tree;
    int* trace;
};
int launch_ens_nuts(alabi_ens* e, double* coords, double* logp, long long step0, long long done0, int K, int thin_by, double* chain,
                    double* chain_logp, long long* n_accept, const NutsInject* inj, hipStream_t s);
int launch_ens_nuts_export(alabi_ens* e, long long step, int depth, int* move, double* e_out, double* z, unsigned* dir, double* u_leaf,
                           double* u_tree, hipStream_t s);
// ens_nuts_adapt.hip: ens_nuts_kernel with a dual-averaged step size per walker (da_state, par, accept_stat as launch_ens_hmc_adapt;
// counts [E*W, 3] and accept_sum [E*W] the caller's), and the initial step-size search of move k_move (ln_e [E*W] in/out)
int launch_ens_nuts_adapt(alabi_ens* e, double* coords, double* logp, long long step0, long long done0, int K, int thin_by, double* chain,
                          double* chain_logp, long long* n_accept, double* da_state, const double* par, long long* counts,
                          double* accept_sum, double* accept_stat, hipStream_t s);
int launch_ens_step_search(alabi_ens* e, const double* coords, const double* logp, long long step, int k_move, double* ln_e, int* iters,
                           hipStream_t s);
int launch_ens_lnprob(alabi_ens* e, const double* coords, int nwalkers, double* logp, int gate_box, hipStream_t s);
int launch_ens_propose(alabi_ens* e, const HalfArgs& args, int nblocks, int gate_box, double* q, double* like, hipStream_t s);
int launch_ens_accept(alabi_ens* e, const HalfArgs& args, int count, const double* q, const double* lp_new, hipStream_t s);
int launch_ens_advance(alabi_ens* e, long long n, hipStream_t s);
// half step of drawn local step t on list slice [begin, end) of `split` in history mode (ens_sharded.hip): rows read from shist / the
// start state, new rows written to `out` (one row of d + 2 doubles per proposal); coords / logp are not modified
int ens_sync_consts(alabi_ens* e, hipStream_t s);   // (inv_len, bounds, prior) on the device match the GP's hyper-parameters
int alabi_ens_half_step_hist(alabi_ens* e, const double* coords, const double* logp, int t, int split, int part_begin, int part_end,
                             const double* shist, double* out, const EnsSwitches& sw, hipStream_t s);
// ens_api.hip: helpers of the handle that ens_run.hip uses
bool ens_draw_ahead_ready(alabi_ens* e);            // second draw-buffer set, side stream and events exist (allocates on first use)
DrawBuffers offset_draws(const DrawBuffers& b, size_t off);
void set_move_args(const alabi_ens* e, HalfArgs& h, size_t t);   // further-partner arrays, move kind and pre-pass buffers of local step t
HalfArgs base_args(alabi_ens* e, double* coords, double* logp);  // ens_run.hip
// ens_stream.hip: the persistent kernel, the version history around a persistent launch (also the group kernel's)
int launch_ens_stream_kernel(alabi_ens* e, const DrawBuffers& rec, int K, int fill_rows, const EnsSwitches& sw, hipStream_t s);
int launch_ens_hist_fill(unsigned long long* rows, size_t words, hipStream_t s);
int launch_ens_call_prologue(alabi_ens* e, const double* coords, const double* logp, const long long* n_accept, bool row0, hipStream_t s);
int launch_ens_stream_epilogue(alabi_ens* e, double* coords, double* logp, int K, int thin_by, double* chain, double* chain_logp,
                               long long* n_accept, long long step_next, long long done0, bool clean_prop, bool last, hipStream_t s);
int launch_ens_hist_prologue(alabi_ens* e, double* coords, double* logp, int K, bool fill, hipStream_t s);
int launch_ens_hist_epilogue(alabi_ens* e, double* coords, double* logp, int K, int thin_by, double* chain, double* chain_logp,
                             long long* n_accept, hipStream_t s);
// ens_pair.hip: the pair variant of the persistent kernel (two workgroups per list position, both outcomes of a pending update)
bool ens_pair_ready(alabi_ens* e, bool eligible);   // eligible: EnsRoute::pair of this call
void ens_pair_release(alabi_ens* e);
int launch_ens_pair_kernel(alabi_ens* e, const DrawBuffers& rec, int K, int fill_rows, int prop_fill_rows, bool placed, const EnsSwitches& sw,
                           hipStream_t s);
bool ens_place_ready(alabi_ens* e, bool eligible);   // ens_place.hip; eligible: EnsRoute::place; the caller has checked ens_pair_ready
int launch_ens_place(alabi_ens* e, DrawBuffers& set, int K, bool count, hipStream_t s);   // allocates set.packed_x / set.place on first use
// ens_group.hip
bool ens_group_buffers(alabi_ens* e, const EnsSwitches& sw, hipStream_t s);   // the group kernel's hand-off buffers exist (allocates on first use); false: take another path
int launch_ens_group(alabi_ens* e, double* coords, double* logp, int K, int thin_by, double* chain, double* chain_logp,
                     long long* n_accept, const EnsSwitches& sw, hipStream_t s);
}  // namespace alabi
