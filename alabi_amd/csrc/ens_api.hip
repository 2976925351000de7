// The ensemble handle behind the extern "C" entry points of include/alabi_hip.h: creation and its buffers, the setters, the
// counters and exports, and the test entries that take a step from injected draws.  What runs a chain is in ens_run.hip; the
// layout of a new handle and every route come from ens_plan.hip.
#include <atomic>
#include <cmath>
#include <cstring>
#include <new>

#include "gp_device.hpp"

using namespace alabi;

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

namespace alabi {

static void free_draws(DrawBuffers& b) {
    if (b.order) (void)hipFree(b.order);
    if (b.cw) (void)hipFree(b.cw);
    if (b.zz) (void)hipFree(b.zz);
    if (b.lnfac) (void)hipFree(b.lnfac);
    if (b.lnu) (void)hipFree(b.lnu);
    if (b.partner) (void)hipFree(b.partner);
    if (b.u_z) (void)hipFree(b.u_z);
    if (b.u_acc) (void)hipFree(b.u_acc);
    if (b.packed) (void)hipFree(b.packed);
    if (b.pos_of) (void)hipFree(b.pos_of);
    if (b.link) (void)hipFree(b.link);
    if (b.packed_x) (void)hipFree(b.packed_x);
    if (b.place) (void)hipFree(b.place);
    b = DrawBuffers{};
}

static hipError_t alloc_draws(DrawBuffers& b, size_t n) {
    hipError_t err = hipSuccess;
    if (err == hipSuccess) err = hipMalloc(&b.order, n * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&b.cw, n * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&b.zz, n * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&b.lnfac, n * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&b.lnu, n * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&b.partner, n * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&b.u_z, n * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&b.u_acc, n * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&b.packed, 4 * n * sizeof(unsigned long long));
    if (err == hipSuccess) err = hipMalloc(&b.pos_of, n * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&b.link, 2 * n * sizeof(unsigned long long));
    return err;
}

// Second set of draw buffers, side stream and events for drawing one chunk ahead; created on the first multi-chunk stream call.
// Not available (single buffer, draws on the main stream) when the set would be large or anything fails to allocate.
bool ens_draw_ahead_ready(alabi_ens* e) {
    if (e->draws2_state != 0) return e->draws2_state > 0;
    e->draws2_state = -1;
    const size_t n = (size_t)e->chunk_cap * e->W * e->E;
    if (n > ((size_t)1 << 20)) return false;                       // 104 bytes per record: at most 109 MB
    bool ok = alloc_draws(e->draws2, n) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&e->side_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&e->ev_free, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&e->ev_drawn, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        free_draws(e->draws2);
        if (e->side_stream) { (void)hipStreamDestroy(e->side_stream); e->side_stream = nullptr; }
        if (e->ev_free) { (void)hipEventDestroy(e->ev_free); e->ev_free = nullptr; }
        if (e->ev_drawn) { (void)hipEventDestroy(e->ev_drawn); e->ev_drawn = nullptr; }
        return false;
    }
    e->draws2_state = 1;
    return true;
}

static void free_move_buffers(MoveBuffers& m) {
    if (m.cw2) (void)hipFree(m.cw2);
    if (m.partner2) (void)hipFree(m.partner2);
    if (m.move) (void)hipFree(m.move);
    if (m.cw3) (void)hipFree(m.cw3);
    if (m.partner3) (void)hipFree(m.partner3);
    if (m.kind) (void)hipFree(m.kind);
    if (m.par) (void)hipFree(m.par);
    m = MoveBuffers{};
}

static void free_kde_buffers(KdeBuffers& k) {
    if (k.white) (void)hipFree(k.white);
    if (k.L) (void)hipFree(k.L);
    if (k.mean) (void)hipFree(k.mean);
    if (k.flag) (void)hipFree(k.flag);
    if (k.singular) (void)hipFree(k.singular);
    k = KdeBuffers{};
}

// The second-partner arrays of the records (first buffer set), allocated when a move set is first given or a DE step is injected;
// the third-partner arrays when the set holds a snooker move or a snooker step is injected.
static int ensure_move_buffers(alabi_ens* e, bool third = false, bool whole_half = false) {
    const size_t n = (size_t)e->chunk_cap * e->W * e->E;
    hipError_t err = hipSuccess;
    if (!e->mv.cw2) {
        err = hipMalloc(&e->mv.cw2, n * sizeof(int));
        if (err == hipSuccess) err = hipMalloc(&e->mv.partner2, n * sizeof(int));
        if (err == hipSuccess) err = hipMalloc(&e->mv.move, (size_t)e->chunk_cap * e->E * sizeof(int));
    }
    if (third && !e->mv.cw3 && err == hipSuccess) {
        err = hipMalloc(&e->mv.cw3, n * sizeof(int));
        if (err == hipSuccess) err = hipMalloc(&e->mv.partner3, n * sizeof(int));
    }
    if (whole_half && !e->mv.kind && err == hipSuccess) {
        err = hipMalloc(&e->mv.kind, (size_t)e->chunk_cap * e->E * sizeof(int));
        if (err == hipSuccess) err = hipMalloc(&e->mv.par, (size_t)e->chunk_cap * e->E * 2 * sizeof(double));
    }
    if (err != hipSuccess) { free_move_buffers(e->mv); return hip_fail(err, "hipMalloc(move buffers)", __FILE__, __LINE__); }
    return ALABI_OK;
}

// What the KDE pre-pass leaves for the half-step kernels: whitened rows of the larger half, factor, mean, flag and the counter.
static int ensure_kde_buffers(alabi_ens* e) {
    if (e->kde.white) return ALABI_OK;
    const size_t E = (size_t)e->E, d = (size_t)e->d, ncmax = (size_t)(e->W + 1) / 2;
    hipError_t err = hipMalloc(&e->kde.white, E * ncmax * d * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&e->kde.L, E * d * d * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&e->kde.mean, E * d * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&e->kde.flag, E * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&e->kde.singular, sizeof(unsigned long long));
    if (err == hipSuccess) err = hipMemset(e->kde.flag, 0, E * sizeof(int));
    if (err == hipSuccess) err = hipMemset(e->kde.singular, 0, sizeof(unsigned long long));
    if (err != hipSuccess) { free_kde_buffers(e->kde); return hip_fail(err, "hipMalloc(KDE buffers)", __FILE__, __LINE__); }
    return ALABI_OK;
}

// The further-partner arrays and, for a set with a walk or KDE move, the step's kind and the pre-pass buffers, offset to local step t
void set_move_args(const alabi_ens* e, HalfArgs& h, size_t t) {
    const size_t WT = (size_t)e->W * e->E;
    h.cw2 = e->has_de ? e->mv.cw2 + t * WT : nullptr;
    h.cw3 = (e->has_snooker || e->has_wk) ? e->mv.cw3 + t * WT : nullptr;
    h.mvkind = e->has_wk ? e->mv.kind + t * e->E : nullptr;
    h.mvpar = e->has_wk ? e->mv.par + 2 * t * e->E : nullptr;
    h.kde = e->kde;
    h.seed = e->seed;
    h.mvidx = e->has_gauss ? e->mv.move + t * e->E : nullptr;
    h.gauss_C = e->has_gauss ? e->gauss_C : nullptr;
    h.gauss_diag = e->gauss_diag;
}

DrawBuffers offset_draws(const DrawBuffers& b, size_t off) {
    DrawBuffers r = b;
    r.order += off; r.cw += off; r.zz += off; r.lnfac += off; r.lnu += off;
    r.partner += off; r.u_z += off; r.u_acc += off; r.packed += 4 * off; r.pos_of += off; r.link += 2 * off;
    if (r.packed_x) r.packed_x += 4 * off;
    if (r.place) r.place += off;
    return r;
}

// (inv_len, lo, hi) live in device memory; refreshed whenever the GP's hyper-parameters changed.
int ens_sync_consts(alabi_ens* e, hipStream_t s) {
    // squared exponential: the half-step kernels read the centred inputs and h = |x - c|^2 / 2 - ln|alpha| (ens_se_prepare; per GP,
    // rebuilt when the inputs, y or the hyper-parameters moved) -- here, i.e. before any stream capture
    if (e->gp->kf.type == 0 && e->gp->has_alpha) { const int st = ens_se_prepare(e->gp, s); if (st != ALABI_OK) return st; }
    if (e->consts_gen == e->gp->gen) return ALABI_OK;
    double host[5 * ALABI_MAX_DIM];
    for (int k = 0; k < ALABI_MAX_DIM; ++k) {
        host[k] = e->gp->inv_len.v[k];
        host[ALABI_MAX_DIM + k] = e->lo[k];
        host[2 * ALABI_MAX_DIM + k] = e->hi[k];
        host[3 * ALABI_MAX_DIM + k] = e->prior_mean[k];
        host[4 * ALABI_MAX_DIM + k] = e->prior_istd[k];
    }
    ALABI_HIP_CHECK(hipMemcpyAsync(e->consts, host, sizeof(host), hipMemcpyHostToDevice, s));
    ALABI_HIP_CHECK(hipStreamSynchronize(s));  // `host` is a stack buffer
    e->consts_gen = e->gp->gen;
    return ALABI_OK;
}

}  // namespace alabi

extern "C" {

// alabi_ens_create and alabi_ens_create_metropolis: the same handle, they differ in the fewest walkers they take (min_w)
static int ens_create(alabi_gp* gp, int W, int min_w, int d, int n_ensembles, const double* bounds, unsigned long long seed, alabi_ens** out) {
    if (!gp || !out || !bounds || W < min_w || W > 8192 || d != gp->d || n_ensembles < 1 || n_ensembles > 4096)
        return ALABI_BAD_ARGUMENT;
    if ((long long)W * n_ensembles > (1LL << 22)) return ALABI_BAD_ARGUMENT;
    alabi_ens* e = new (std::nothrow) alabi_ens();
    if (!e) return ALABI_BAD_ARGUMENT;
    e->gp = gp; e->W = W; e->d = d; e->E = n_ensembles; e->seed = seed;
    { static std::atomic<long long> next_serial{0}; e->serial = ++next_serial; }
    for (int k = 0; k < ALABI_MAX_DIM; ++k) {
        e->lo[k] = (k < d) ? bounds[2 * k] : 0.0;
        e->hi[k] = (k < d) ? bounds[2 * k + 1] : 0.0;
    }
    // workgroup size, chunk length and the persistent kernel's grid: ens_create_plan, under the switches as they stand now
    e->n_cu = device_cu_count();
    const EnsCreatePlan plan = ens_create_plan(W, n_ensembles, gp->Npad, e->n_cu, ens_switches());
    e->threads = plan.threads;
    e->chunk_cap = plan.chunk_cap;
    const long long WT = (long long)W * n_ensembles;
    const size_t n = (size_t)e->chunk_cap * WT;
    DrawBuffers& b = e->draws;
    hipError_t err = alloc_draws(b, n);
    if (err == hipSuccess) err = hipMalloc(&e->run_state, 4 * sizeof(long long));
    if (err == hipSuccess) err = hipMalloc(&e->consts, 5 * ALABI_MAX_DIM * sizeof(double));
    // persistent dataflow path: one workgroup per list position, all co-resident (at most one per CU)
    if (plan.stream_grid > 0) {
        e->stream_grid = plan.stream_grid;
        const size_t hist_words = ((size_t)e->chunk_cap + 1) * WT * (d + 2);   // row = coords, logp, accepted
        const size_t state_words = 1 + (size_t)WT * (d + 1);                   // err | coords | logp
        if (err == hipSuccess) err = hipMalloc(&e->hist, hist_words * sizeof(unsigned long long));
        if (err == hipSuccess) err = hipMalloc(&e->state_dev, state_words * sizeof(unsigned long long));
        if (err == hipSuccess) err = hipMemset(e->state_dev, 0, state_words * sizeof(unsigned long long));
        if (err == hipSuccess) err = hipHostMalloc(reinterpret_cast<void**>(&e->state_host), state_words * sizeof(unsigned long long), hipHostMallocDefault);
        if (err == hipSuccess) err = hipMalloc(&e->save, (size_t)WT * (d + 1) * sizeof(double) + (size_t)WT * sizeof(long long));
        if (err == hipSuccess) e->err = reinterpret_cast<int*>(e->state_dev);
        e->stream_ok = (err == hipSuccess) ? 1 : 0;
    }
    if (err != hipSuccess) {
        alabi_ens_destroy(e);
        return hip_fail(err, "hipMalloc(ensemble buffers)", __FILE__, __LINE__);
    }
    *out = e;
    return ALABI_OK;
}

int alabi_ens_create(alabi_gp* gp, int W, int d, int n_ensembles, const double* bounds, unsigned long long seed,
                     alabi_ens** out) {
    return ens_create(gp, W, 2, d, n_ensembles, bounds, seed, out);
}

// A handle for Metropolis sets: one walker is enough.  With W < 2 every entry that would draw a red-blue record refuses a table
// that is not all Gaussian (alabi_ens_set_moves, alabi_ens_run, alabi_ens_draw).
int alabi_ens_create_metropolis(alabi_gp* gp, int W, int d, int n_ensembles, const double* bounds, unsigned long long seed,
                                alabi_ens** out) {
    return ens_create(gp, W, 1, d, n_ensembles, bounds, seed, out);
}

int alabi_ens_destroy(alabi_ens* e) {
    if (!e) return ALABI_OK;
    if (e->graph_exec) (void)hipGraphExecDestroy(e->graph_exec);
    if (e->side_stream) (void)hipStreamSynchronize(e->side_stream);   // draws made ahead for a call that never came
    free_draws(e->draws);
    free_draws(e->draws2);
    free_move_buffers(e->mv);
    free_kde_buffers(e->kde);
    if (e->gauss_C) (void)hipFree(e->gauss_C);
    if (e->nuts_counts) (void)hipFree(e->nuts_counts);
    if (e->nuts_accept) (void)hipFree(e->nuts_accept);
    if (e->side_stream) (void)hipStreamDestroy(e->side_stream);
    if (e->ev_free) (void)hipEventDestroy(e->ev_free);
    if (e->ev_drawn) (void)hipEventDestroy(e->ev_drawn);
    if (e->run_state) (void)hipFree(e->run_state);
    if (e->consts) (void)hipFree(e->consts);
    if (e->hist) (void)hipFree(e->hist);
    if (e->part) (void)hipFree(e->part);
    if (e->cand) (void)hipFree(e->cand);
    if (e->state_dev) (void)hipFree(e->state_dev);       // e->err is its first word
    if (e->state_host) (void)hipHostFree(e->state_host);
    if (e->save) (void)hipFree(e->save);
    ens_pair_release(e);
    delete e;
    return ALABI_OK;
}

int alabi_ens_set_normal_prior(alabi_ens* e, const double* mean, const double* std) {
    if (!e || !mean || !std) return ALABI_BAD_ARGUMENT;
    e->has_prior = 0; e->prior_const = 0.0;
    for (int k = 0; k < ALABI_MAX_DIM; ++k) { e->prior_mean[k] = 0.0; e->prior_istd[k] = 0.0; }
    for (int k = 0; k < e->d; ++k) {
        if (std::isfinite(mean[k]) && std::isfinite(std[k]) && std[k] > 0.0) {
            e->prior_mean[k] = mean[k];
            e->prior_istd[k] = 1.0 / std[k];
            e->prior_const += -std::log(std[k]) - 0.9189385332046727;   // -log(std) - log(2 pi) / 2, as norm.logpdf
            e->has_prior = 1;
        }
    }
    e->consts_gen = -1;                                                  // re-upload
    e->settings_gen++;
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }
    return ALABI_OK;
}

int alabi_ens_set_logp_affine(alabi_ens* e, double scale, double shift) {
    if (!e || !(scale > 0.0) || !std::isfinite(scale) || !std::isfinite(shift)) return ALABI_BAD_ARGUMENT;
    e->lp_scale = scale; e->lp_shift = shift;
    e->settings_gen++;
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }   // captured launches carry the old values
    return ALABI_OK;
}

int alabi_ens_set_logp_map(alabi_ens* e, int kind) {
    if (!e || kind < 0 || kind > 2) return ALABI_BAD_ARGUMENT;
    e->ymap = kind;
    e->settings_gen++;
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }   // captured launches carry the old value
    return ALABI_OK;
}

int alabi_ens_set_moves(alabi_ens* e, int n, const int* kind, const double* cum, const double* p0, const double* p1) {
    if (!e || n < 0 || n > ALABI_MAX_MOVES || (n > 0 && (!kind || !cum || !p0 || !p1))) return ALABI_BAD_ARGUMENT;
    MoveTable mt{};
    bool de = false, snooker = false, walk = false, kde = false, gauss = false, all_gauss = n > 0, hmc = false, all_hmc = n > 0, nuts = false, all_nuts = n > 0;
    const int nc_min = e->W / 2, nc_max = (e->W + 1) / 2;   // the two complementary halves
    double prev = 0.0;
    for (int k = 0; k < n; ++k) {
        if (!(cum[k] >= prev) || !std::isfinite(cum[k])) return ALABI_BAD_ARGUMENT;   // cumulative weights do not decrease
        prev = cum[k];
        if (kind[k] == 0) { if (!(p0[k] > 1.0) || !std::isfinite(p0[k])) return ALABI_BAD_ARGUMENT; }          // stretch: a > 1
        else if (kind[k] == 1) { if (!std::isfinite(p0[k]) || !std::isfinite(p1[k])) return ALABI_BAD_ARGUMENT; de = true; }
        else if (kind[k] == 2) { if (!std::isfinite(p0[k])) return ALABI_BAD_ARGUMENT; snooker = true; }                // snooker: gammas
        else if (kind[k] == 3) {                             // walk: p0 = s0 (0: the whole half), 2 <= s0 <= the smaller half
            const double s0 = p0[k] == 0.0 ? (double)nc_min : p0[k];
            if (!(s0 >= 2.0) || !(s0 <= (double)nc_min) || s0 != std::floor(s0) || nc_max > 2048) return ALABI_BAD_ARGUMENT;
            walk = true;
        } else if (kind[k] == 4) {                           // KDE: the bandwidth factors of the two splits; more rows than dimensions
            if (!(p0[k] > 0.0) || !std::isfinite(p0[k]) || !(p1[k] > 0.0) || !std::isfinite(p1[k]) || nc_min < e->d + 1) return ALABI_BAD_ARGUMENT;
            kde = true;
        } else if (kind[k] == 5) {                           // Gaussian: p0 = ln factor >= 0 (0: none), p1 = mode 0 / 1 / 2
            if (!(p0[k] >= 0.0) || !std::isfinite(p0[k]) || !(p1[k] == 0.0 || p1[k] == 1.0 || p1[k] == 2.0)) return ALABI_BAD_ARGUMENT;
            // its scale factor has been handed over for this slot (alabi_ens_set_move_scale), diagonal where one coordinate moves
            if (!((e->gauss_staged >> k) & 1) || (p1[k] != 0.0 && !((e->gauss_diag >> k) & 1))) return ALABI_BAD_ARGUMENT;
            gauss = true;
        } else if (kind[k] == 6) {                           // HMC: p0 = step size > 0, p1 = n_leapfrog (1 ... 64) + ln jitter / 512
            if (!(p0[k] > 0.0) || !std::isfinite(p0[k]) || !std::isfinite(p1[k]) || !(p1[k] >= 1.0) || !(p1[k] < 65.0)) return ALABI_BAD_ARGUMENT;
            if (!((e->gauss_staged >> k) & 1)) return ALABI_BAD_ARGUMENT;   // its scale factor has been handed over for this slot
            hmc = true;
        } else if (kind[k] == 7) {                           // NUTS: p0 = step size > 0, p1 = max_depth (1 ... 10) + ln jitter / 512
            if (!(p0[k] > 0.0) || !std::isfinite(p0[k]) || !std::isfinite(p1[k]) || !(p1[k] >= 1.0) || !(p1[k] < ALABI_NUTS_MAX_DEPTH + 1.0))
                return ALABI_BAD_ARGUMENT;
            if (!((e->gauss_staged >> k) & 1)) return ALABI_BAD_ARGUMENT;   // its scale factor has been handed over for this slot
            nuts = true;
        }
        else return ALABI_BAD_ARGUMENT;
        if (kind[k] != 5) all_gauss = false;
        if (kind[k] != 6) all_hmc = false;
        if (kind[k] != 7) all_nuts = false;
        mt.kind[k] = kind[k]; mt.cum[k] = cum[k]; mt.p0[k] = p0[k]; mt.p1[k] = p1[k];
    }
    if (n > 0 && !(prev > 0.0)) return ALABI_BAD_ARGUMENT;
    if (hmc && !all_hmc) return ALABI_BAD_ARGUMENT;      // an HMC move runs on ens_hmc_kernel alone: no mixture with another kind
    if (nuts && !all_nuts) return ALABI_BAD_ARGUMENT;    // nor does a NUTS move: ens_nuts_kernel alone
    if (e->W < 2 && !all_gauss && !all_hmc && !all_nuts) return ALABI_BAD_ARGUMENT;   // a red-blue move needs a complementary half
    if (de && e->W < 4) return ALABI_BAD_ARGUMENT;       // two distinct partners in a complementary list of W / 2 walkers
    if (snooker && e->W < 6) return ALABI_BAD_ARGUMENT;  // three distinct partners
    if (nuts && !e->nuts_counts) {                       // the per-walker sums of alabi_ens_nuts_stats, zero from here
        const size_t WT = (size_t)e->W * e->E;
        ALABI_HIP_CHECK(hipMalloc(&e->nuts_counts, WT * 3 * sizeof(long long)));
        ALABI_HIP_CHECK(hipMemset(e->nuts_counts, 0, WT * 3 * sizeof(long long)));
        ALABI_HIP_CHECK(hipMalloc(&e->nuts_accept, WT * sizeof(double)));
        ALABI_HIP_CHECK(hipMemset(e->nuts_accept, 0, WT * sizeof(double)));
    }
    if (n > 0 && !hmc && !nuts) { const int st = ensure_move_buffers(e, snooker || walk || kde || gauss, walk || kde || gauss); if (st != ALABI_OK) return st; }
    if (kde) { const int st = ensure_kde_buffers(e); if (st != ALABI_OK) return st; }
    mt.n = n;
    e->moves = mt;
    e->has_de = de || snooker || walk || kde || gauss;   // more than one partner row, or none: one launch per half step
    e->has_snooker = snooker;
    e->has_wk = walk || kde || gauss;                    // proposals formed where they are used: the whole-half instantiations
    e->has_kde = kde;
    e->has_gauss = gauss; e->all_gauss = gauss && all_gauss;
    e->all_hmc = hmc && all_hmc;
    e->all_nuts = nuts && all_nuts;
    e->gauss_staged = 0;                                 // scale factors belong to the table they were handed over for
    e->drawn_n = 0;                                      // records drawn under the old move set are not the new set's
    e->ahead_valid = false;                              // nor are those made ahead for the next stream call
    e->moves_gen++;
    e->settings_gen++;
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }   // captured draw launches carry the old table
    return ALABI_OK;
}

int alabi_ens_set_move_scale(alabi_ens* e, int k, const double* C, int diagonal) {
    if (!e || !C || k < 0 || k >= ALABI_MAX_MOVES) return ALABI_BAD_ARGUMENT;
    const int d = e->d;
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
            const double v = C[(size_t)i * d + j];
            if (!std::isfinite(v) || (j > i && v != 0.0) || (diagonal && j != i && v != 0.0) || (j == i && !(v > 0.0))) return ALABI_BAD_ARGUMENT;
        }
    // slot k of the current table is in use by a Gaussian move that moves one coordinate per step: a diagonal factor, as in emcee
    if (k < e->moves.n && e->moves.kind[k] == 5 && e->moves.p1[k] != 0.0 && !diagonal) return ALABI_BAD_ARGUMENT;
    if (!e->gauss_C) {
        hipError_t err = hipMalloc(&e->gauss_C, (size_t)ALABI_MAX_MOVES * ALABI_MAX_DIM * ALABI_MAX_DIM * sizeof(double));
        if (err != hipSuccess) { e->gauss_C = nullptr; return hip_fail(err, "hipMalloc(move scale factors)", __FILE__, __LINE__); }
    }
    ALABI_HIP_CHECK(hipDeviceSynchronize());               // nothing in flight reads the old factor
    ALABI_HIP_CHECK(hipMemcpy(e->gauss_C + (size_t)k * d * d, C, (size_t)d * d * sizeof(double), hipMemcpyHostToDevice));
    e->gauss_staged |= 1 << k;
    if (diagonal) e->gauss_diag |= 1 << k; else e->gauss_diag &= ~(1 << k);
    e->settings_gen++;
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }   // captured launches carry gauss_diag
    return ALABI_OK;
}

int alabi_ens_mh_plan(alabi_ens* e, int* out) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    for (int i = 0; i < 4; ++i) out[i] = e->mh_plan[i];
    return ALABI_OK;
}

int alabi_ens_set_stream(alabi_ens* e, int enabled) {
    if (!e) return ALABI_BAD_ARGUMENT;
    // The switch belongs to the handle, not to the move table: it covers the persistent kernels of a red-blue table (they need
    // the version history) and ens_mh_kernel of an all-Gaussian one (it needs nothing), whichever table the next run finds.
    const bool can_stream = e->hist && e->err;
    if (enabled && !can_stream && !e->all_gauss && !e->all_hmc && !e->all_nuts) return ALABI_BAD_ARGUMENT;
    e->mh_ok = enabled ? 1 : 0;
    e->stream_ok = (enabled && can_stream) ? 1 : 0;
    e->settings_gen++;
    return ALABI_OK;
}

int alabi_ens_stream_variant(alabi_ens* e, int* variant) {
    if (!e || !variant) return ALABI_BAD_ARGUMENT;
    *variant = (e->last_path == 1) ? e->last_variant : 0;
    return ALABI_OK;
}

// The pair kernel's debug counters (alabi_ens::pair_stats); counting starts with the next run
static int pair_stats_alloc(alabi_ens* e) {
    if (e->pair_stats) return ALABI_OK;
    ALABI_HIP_CHECK(hipMalloc(&e->pair_stats, ALABI_PAIR_STATS_WORDS * sizeof(unsigned long long)));
    ALABI_HIP_CHECK(hipMemset(e->pair_stats, 0, ALABI_PAIR_STATS_WORDS * sizeof(unsigned long long)));
    return ALABI_OK;
}

int alabi_ens_pair_stats(alabi_ens* e, long long* out, int reset) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    int st;
    if ((st = pair_stats_alloc(e)) != ALABI_OK) return st;
    ALABI_HIP_CHECK(hipDeviceSynchronize());
    ALABI_HIP_CHECK(hipMemcpy(out, e->pair_stats, 9 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) ALABI_HIP_CHECK(hipMemset(e->pair_stats, 0, 9 * sizeof(unsigned long long)));
    return ALABI_OK;
}

int alabi_ens_place_stats(alabi_ens* e, long long* out, int reset) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    out[0] = e->place_state > 0; out[1] = out[2] = 0;
    if (!e->place_stats) return ALABI_OK;
    ALABI_HIP_CHECK(hipDeviceSynchronize());
    ALABI_HIP_CHECK(hipMemcpy(out + 1, e->place_stats, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) ALABI_HIP_CHECK(hipMemset(e->place_stats, 0, 2 * sizeof(unsigned long long)));
    return ALABI_OK;
}

int alabi_ens_export_placement(alabi_ens* e, long long step0, int nsteps, double a, int* place, unsigned long long* packed,
                               unsigned long long* packed_x, void* stream) {
    if (!e || !place || nsteps <= 0 || nsteps > e->chunk_cap || !(a > 1.0)) return ALABI_BAD_ARGUMENT;
    if (e->place_state <= 0) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = launch_ens_draw_at(e, e->draws, nsteps, a, false, step0, s)) != ALABI_OK) return st;
    if ((st = launch_ens_place(e, e->draws, nsteps, false, s)) != ALABI_OK) return st;
    e->drawn_n = 0;                                   // (the buffers no longer hold what alabi_ens_draw put there)
    const size_t n = (size_t)nsteps * e->W * e->E;
    ALABI_HIP_CHECK(hipMemcpyAsync(place, e->draws.place, n * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (packed) ALABI_HIP_CHECK(hipMemcpyAsync(packed, e->draws.packed, 4 * n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    if (packed_x) ALABI_HIP_CHECK(hipMemcpyAsync(packed_x, e->draws.packed_x, 4 * n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    return ALABI_OK;
}

int alabi_ens_pair_stats2(alabi_ens* e, long long* out, int enable) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    int st;
    if (enable && (st = pair_stats_alloc(e)) != ALABI_OK) return st;
    for (int i = 0; i < 6; ++i) out[i] = 0;
    if (!e->pair_stats) return ALABI_OK;
    ALABI_HIP_CHECK(hipDeviceSynchronize());
    ALABI_HIP_CHECK(hipMemcpy(out, e->pair_stats + 9, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    ALABI_HIP_CHECK(hipMemset(e->pair_stats + 9, 0, 6 * sizeof(unsigned long long)));
    return ALABI_OK;
}

int alabi_ens_pair_stats3(alabi_ens* e, long long* out, int enable) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    int st;
    if (enable && (st = pair_stats_alloc(e)) != ALABI_OK) return st;
    for (int i = 0; i < 20; ++i) out[i] = 0;
    if (!e->pair_stats) return ALABI_OK;
    ALABI_HIP_CHECK(hipDeviceSynchronize());
    long long raw[20];                                // per role, by lane of the kernel's counter: [0] verdict looks, [2..4] verdict bins,
                                                      // [5] input looks, [6] inputs complete without a reload, [7..9] input bins
    ALABI_HIP_CHECK(hipMemcpy(raw, e->pair_stats + 16, 20 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int r = 0; r < 2; ++r) {
        const long long* q = raw + 10 * r;
        long long* o = out + 10 * r;
        o[0] = q[2] + q[3] + q[4]; o[1] = q[0]; o[2] = q[2]; o[3] = q[3]; o[4] = q[4];
        o[5] = q[7] + q[8] + q[9]; o[6] = q[5]; o[7] = q[7]; o[8] = q[8]; o[9] = q[9];
    }
    ALABI_HIP_CHECK(hipMemset(e->pair_stats + 16, 0, 20 * sizeof(unsigned long long)));
    return ALABI_OK;
}

int alabi_ens_last_path(alabi_ens* e, int* path) {
    if (!e || !path) return ALABI_BAD_ARGUMENT;
    *path = e->last_path;
    return ALABI_OK;
}

int alabi_ens_group_plan(alabi_ens* e, int* out) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    for (int i = 0; i < 8; ++i) out[i] = e->group_plan[i];
    return ALABI_OK;
}

int alabi_ens_lnprob(alabi_ens* e, const double* coords, double* logp, void* stream) {
    if (!e || !coords || !logp) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    int st = ens_sync_consts(e, as_stream(stream));
    if (st != ALABI_OK) return st;
    return launch_ens_lnprob(e, coords, e->W * e->E, logp, 1, as_stream(stream));
}

int alabi_ens_surrogate(alabi_ens* e, const double* points, int M, double* like, void* stream) {
    if (!e || !points || !like || M < 0) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    if (M == 0) return ALABI_OK;
    int st = ens_sync_consts(e, as_stream(stream));
    if (st != ALABI_OK) return st;
    // the normal-prior rows are part of the fused log-probability, not of the surrogate: evaluate without them
    const int hp = e->has_prior; const double pc = e->prior_const;
    e->has_prior = 0; e->prior_const = 0.0;
    st = launch_ens_lnprob(e, points, M, like, 0, as_stream(stream));
    e->has_prior = hp; e->prior_const = pc;
    return st;
}

int alabi_ens_boundary_stats(alabi_ens* e, long long* out) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    for (int i = 0; i < 4; ++i) out[i] = e->boundary_stats[i];
    return ALABI_OK;
}

int alabi_ens_propose(alabi_ens* e, const double* coords, int t, int split, int gate_box, double* q, double* like,
                      void* stream) {
    if (!e || !coords || !q || t < 0 || t >= e->drawn_n || (split != 0 && split != 1) || e->E != 1) return ALABI_BAD_ARGUMENT;
    if (like && (!e->gp->computed || !e->gp->has_alpha)) return ALABI_NOT_COMPUTED;
    int st = ens_sync_consts(e, as_stream(stream));
    if (st != ALABI_OK) return st;
    HalfArgs h = base_args(e, const_cast<double*>(coords), nullptr);
    const int nS = split == 0 ? h.n0 : e->W - h.n0;
    h.rec = offset_draws(e->draws, (size_t)t * e->W);
    set_move_args(e, h, (size_t)t);
    h.local_t = t; h.split = split; h.part_begin = 0;
    if (e->has_kde && nS > 0 && (st = launch_ens_kde_prepass(e, h, as_stream(stream))) != ALABI_OK) return st;
    return launch_ens_propose(e, h, nS, gate_box, q, like, as_stream(stream));
}

int alabi_ens_accept(alabi_ens* e, double* coords, double* logp, int t, int split, const double* q, const double* lp_new,
                     long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !q || !lp_new || t < 0 || t >= e->drawn_n || (split != 0 && split != 1) || e->E != 1)
        return ALABI_BAD_ARGUMENT;
    HalfArgs h = base_args(e, coords, logp);
    const int nS = split == 0 ? h.n0 : e->W - h.n0;
    h.rec = offset_draws(e->draws, (size_t)t * e->W);
    h.local_t = t; h.split = split; h.part_begin = 0; h.n_accept = n_accept;
    return launch_ens_accept(e, h, nS, q, lp_new, as_stream(stream));
}

int alabi_ens_step_lists(alabi_ens* e, int t, int* order_out, int* n0, void* stream) {
    if (!e || t < 0 || t >= e->drawn_n || !order_out || !n0 || e->E != 1) return ALABI_BAD_ARGUMENT;
    ALABI_HIP_CHECK(hipMemcpyAsync(order_out, e->draws.order + (size_t)t * e->W, (size_t)e->W * sizeof(int),
                                   hipMemcpyDeviceToDevice, as_stream(stream)));
    *n0 = (e->W + 1) / 2;
    return ALABI_OK;
}

int alabi_ens_step_with_randoms(alabi_ens* e, double* coords, double* logp, const int* order, int n0,
                                const double* u_z, const int* partner, const double* u_acc, double a,
                                long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !order || !u_z || !partner || !u_acc || n0 < 0 || n0 > e->W || !(a > 1.0) || e->E != 1)
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = ens_sync_consts(e, s)) != ALABI_OK) return st;
    if ((st = launch_ens_prep(e, order, n0, u_z, partner, u_acc, a, s)) != ALABI_OK) return st;
    e->drawn_n = 0;  // row 0 of the draw buffers now holds caller data
    const EnsSwitches sw = ens_switches();
    HalfArgs h = base_args(e, coords, logp);
    h.rec = e->draws; h.n0 = n0; h.n_accept = n_accept; h.local_t = 0; h.part_begin = 0;
    h.split = 0;
    if ((st = launch_ens_half_args(e, h, n0, sw, s)) != ALABI_OK) return st;
    h.split = 1;
    return launch_ens_half_args(e, h, e->W - n0, sw, s);
}

int alabi_ens_step_with_randoms_de(alabi_ens* e, double* coords, double* logp, const int* order, int n0, const int* j1,
                                   const int* j2, const double* gamma, const double* u_acc, long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !order || !j1 || !j2 || !gamma || !u_acc || n0 < 0 || n0 > e->W || e->E != 1)
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = ens_sync_consts(e, s)) != ALABI_OK) return st;
    if ((st = ensure_move_buffers(e)) != ALABI_OK) return st;
    if ((st = launch_ens_prep_de(e, order, n0, j1, j2, gamma, u_acc, s)) != ALABI_OK) return st;
    e->drawn_n = 0;  // row 0 of the draw buffers now holds caller data
    const EnsSwitches sw = ens_switches();
    HalfArgs h = base_args(e, coords, logp);
    h.rec = e->draws; h.cw2 = e->mv.cw2; h.n0 = n0; h.n_accept = n_accept; h.local_t = 0; h.part_begin = 0;
    h.split = 0;
    if ((st = launch_ens_half_args(e, h, n0, sw, s)) != ALABI_OK) return st;
    h.split = 1;
    return launch_ens_half_args(e, h, e->W - n0, sw, s);
}

int alabi_ens_step_with_randoms_snooker(alabi_ens* e, double* coords, double* logp, const int* order, int n0, const int* j1,
                                        const int* j2, const int* j3, double gamma, const double* u_acc, long long* n_accept,
                                        void* stream) {
    if (!e || !coords || !logp || !order || !j1 || !j2 || !j3 || !u_acc || !std::isfinite(gamma) || n0 < 0 || n0 > e->W || e->E != 1)
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = ens_sync_consts(e, s)) != ALABI_OK) return st;
    if ((st = ensure_move_buffers(e, true)) != ALABI_OK) return st;
    if ((st = launch_ens_prep_snooker(e, order, n0, j1, j2, j3, gamma, u_acc, s)) != ALABI_OK) return st;
    e->drawn_n = 0;  // row 0 of the draw buffers now holds caller data
    const EnsSwitches sw = ens_switches();
    HalfArgs h = base_args(e, coords, logp);
    h.rec = e->draws; h.cw2 = e->mv.cw2; h.cw3 = e->mv.cw3; h.n0 = n0; h.n_accept = n_accept; h.local_t = 0; h.part_begin = 0;
    h.split = 0;
    if ((st = launch_ens_half_args(e, h, n0, sw, s)) != ALABI_OK) return st;
    h.split = 1;
    return launch_ens_half_args(e, h, e->W - n0, sw, s);
}

// one full step of the whole-half instantiation on row 0 of the draw buffers, from a test entry's draws
static int step_injected_wk(alabi_ens* e, double* coords, double* logp, const int* order, int n0, int kind, double p0, double p1,
                            const WkInject& inj, const double* u_acc, long long* n_accept, hipStream_t s) {
    int st;
    if ((st = ens_sync_consts(e, s)) != ALABI_OK) return st;
    if ((st = ensure_move_buffers(e, true, true)) != ALABI_OK) return st;
    if (kind == 4 && (st = ensure_kde_buffers(e)) != ALABI_OK) return st;
    if ((st = launch_ens_prep_wk(e, order, u_acc, s)) != ALABI_OK) return st;
    if ((st = launch_ens_set_step_move(e, kind, p0, p1, s)) != ALABI_OK) return st;
    e->drawn_n = 0;  // row 0 of the draw buffers now holds caller data
    const EnsSwitches sw = ens_switches();
    HalfArgs h = base_args(e, coords, logp);
    h.rec = e->draws; h.cw2 = e->mv.cw2; h.cw3 = e->mv.cw3; h.mvkind = e->mv.kind; h.mvpar = e->mv.par; h.kde = e->kde; h.seed = e->seed;
    h.inj = inj;
    h.n0 = n0; h.n_accept = n_accept; h.local_t = 0; h.part_begin = 0;
    for (int split = 0; split < 2; ++split) {
        const int nS = split == 0 ? n0 : e->W - n0;
        if (nS == 0) continue;
        h.split = split;
        if (kind == 4 && (st = launch_ens_kde_prepass(e, h, s)) != ALABI_OK) return st;
        if ((st = launch_ens_half_args(e, h, nS, sw, s)) != ALABI_OK) return st;
    }
    return ALABI_OK;
}

int alabi_ens_step_with_randoms_walk(alabi_ens* e, double* coords, double* logp, const int* order, int n0, int s0, const int* subset,
                                     const double* z, const double* u_acc, long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !order || !subset || !z || !u_acc || n0 < 0 || n0 > e->W || e->E != 1) return ALABI_BAD_ARGUMENT;
    // every active half needs s0 rows in the other one, which the kernel's lists must hold
    const int n1 = e->W - n0;
    if (s0 < 2 || (n0 > 0 && s0 > n1) || (n1 > 0 && s0 > n0) || n0 > 2048 || n1 > 2048) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    WkInject inj{subset, z, nullptr};
    return step_injected_wk(e, coords, logp, order, n0, 3, (double)s0, 0.0, inj, u_acc, n_accept, as_stream(stream));
}

int alabi_ens_step_with_randoms_kde(alabi_ens* e, double* coords, double* logp, const int* order, int n0, double factor, const int* r,
                                    const double* z, const double* u_acc, double* lnfac_out, long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !order || !r || !z || !u_acc || n0 < 0 || n0 > e->W || e->E != 1) return ALABI_BAD_ARGUMENT;
    const int n1 = e->W - n0;
    // the pre-pass buffers hold (W + 1) / 2 rows; scipy's gaussian_kde refuses fewer rows than d + 1 as well
    if (!(factor > 0.0) || !std::isfinite(factor) || n0 > (e->W + 1) / 2 || n1 > (e->W + 1) / 2 || n0 < e->d + 1 || n1 < e->d + 1)
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    WkInject inj{r, z, lnfac_out};
    return step_injected_wk(e, coords, logp, order, n0, 4, factor, factor, inj, u_acc, n_accept, as_stream(stream));
}

int alabi_ens_step_with_randoms_gauss(alabi_ens* e, double* coords, double* logp, const int* order, int n0, int k_move, double f,
                                      const int* coord, const double* z, const double* u_acc, long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !order || !coord || !z || !u_acc || n0 < 0 || n0 > e->W || e->E != 1) return ALABI_BAD_ARGUMENT;
    if (k_move < 0 || k_move >= e->moves.n || e->moves.kind[k_move] != 5 || !std::isfinite(f))
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = ens_sync_consts(e, s)) != ALABI_OK) return st;
    if ((st = ensure_move_buffers(e, true, true)) != ALABI_OK) return st;
    if ((st = launch_ens_prep_wk(e, order, u_acc, s)) != ALABI_OK) return st;
    if ((st = launch_ens_set_step_move(e, 5, e->moves.p0[k_move], e->moves.p1[k_move], s)) != ALABI_OK) return st;
    e->drawn_n = 0;  // row 0 of the draw buffers now holds caller data
    const EnsSwitches sw = ens_switches();
    HalfArgs h = base_args(e, coords, logp);
    h.rec = e->draws; h.cw2 = e->mv.cw2; h.cw3 = e->mv.cw3; h.mvkind = e->mv.kind; h.mvpar = e->mv.par; h.kde = e->kde; h.seed = e->seed;
    h.inj = WkInject{coord, z, nullptr};
    h.gauss_C = e->gauss_C; h.gauss_diag = e->gauss_diag; h.gauss_k = k_move; h.gauss_f = f;
    h.n0 = n0; h.n_accept = n_accept; h.local_t = 0; h.part_begin = 0;
    for (int split = 0; split < 2; ++split) {
        const int nS = split == 0 ? n0 : e->W - n0;
        h.split = split;
        if ((st = launch_ens_half_args(e, h, nS, sw, s)) != ALABI_OK) return st;
    }
    return ALABI_OK;
}

int alabi_ens_export_gauss_draws(alabi_ens* e, double* f, int* coord, double* z, void* stream) {
    if (!e || !f || !coord || !z || e->drawn_n < 1 || !e->mv.kind) return ALABI_BAD_ARGUMENT;
    return launch_ens_gauss_export(e, f, coord, z, as_stream(stream));
}

int alabi_ens_hmc_plan(alabi_ens* e, int* out) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    for (int i = 0; i < 4; ++i) out[i] = e->hmc_plan[i];
    return ALABI_OK;
}

int alabi_ens_log_prob_grad(alabi_ens* e, const double* coords, int M, double* logp, double* grad, void* stream) {
    if (!e || !coords || !logp || !grad || M < 0) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    if (M == 0) return ALABI_OK;
    const int st = ens_sync_consts(e, as_stream(stream));
    if (st != ALABI_OK) return st;
    return launch_ens_lp_grad(e, coords, M, logp, grad, as_stream(stream));
}

int alabi_ens_maximize(alabi_ens* e, const double* starts, int S, int maxiter, double gtol, double* x_out, double* lp_out, int* iters_out,
                       int* status_out, double* gnorm_out, double* trace, int ntrace, void* stream) {
    if (!e || !starts || !x_out || !lp_out || !iters_out || !status_out || !gnorm_out || S < 0 || maxiter < 0 || ntrace < 0 ||
        (ntrace > 0 && !trace) || !(gtol >= 0.0))
        return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    if (S == 0) return ALABI_OK;
    const int st = ens_sync_consts(e, as_stream(stream));
    if (st != ALABI_OK) return st;
    return launch_ens_map(e, starts, S, maxiter, gtol, x_out, lp_out, iters_out, status_out, gnorm_out, trace, ntrace, as_stream(stream));
}

int alabi_ens_log_prob_hessian(alabi_ens* e, const double* coords, int M, double* hess, void* stream) {
    if (!e || !coords || !hess || M < 0) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    if (M == 0) return ALABI_OK;
    const int st = ens_sync_consts(e, as_stream(stream));
    if (st != ALABI_OK) return st;
    return launch_ens_lp_hess(e, coords, M, hess, as_stream(stream));
}

int alabi_ens_map_plan(alabi_ens* e, int* out) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    ens_map_plan(e, out);
    return ALABI_OK;
}

int alabi_ens_step_with_randoms_hmc(alabi_ens* e, double* coords, double* logp, int k_move, double eps, const double* z,
                                    const double* u_acc, long long* n_accept, void* stream) {
    if (!e || !coords || !logp || !z || !u_acc || e->E != 1 || !e->all_hmc) return ALABI_BAD_ARGUMENT;
    if (k_move < 0 || k_move >= e->moves.n || !(eps > 0.0) || !std::isfinite(eps)) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    const int st = ens_sync_consts(e, s);
    if (st != ALABI_OK) return st;
    return launch_ens_hmc(e, coords, logp, 0, 0, 1, 1, nullptr, nullptr, n_accept, k_move, eps, z, u_acc, s);
}

int alabi_ens_export_hmc_draws(alabi_ens* e, long long step, int* move, double* eps, double* z, double* u_acc, void* stream) {
    if (!e || !move || !eps || !z || !e->all_hmc) return ALABI_BAD_ARGUMENT;
    return launch_ens_hmc_export(e, step, move, eps, z, u_acc, as_stream(stream));
}

int alabi_ens_nuts_plan(alabi_ens* e, int* out) {
    if (!e || !out) return ALABI_BAD_ARGUMENT;
    for (int i = 0; i < 4; ++i) out[i] = e->nuts_plan[i];
    return ALABI_OK;
}

int alabi_ens_nuts_stats(alabi_ens* e, long long* counts_host, double* accept_host, int reset) {
    if (!e || !counts_host || !accept_host) return ALABI_BAD_ARGUMENT;
    const size_t WT = (size_t)e->W * e->E;
    if (!e->nuts_counts || !e->nuts_accept) {            // no NUTS table yet: nothing has been summed
        for (size_t i = 0; i < WT * 3; ++i) counts_host[i] = 0;
        for (size_t i = 0; i < WT; ++i) accept_host[i] = 0.0;
        return ALABI_OK;
    }
    ALABI_HIP_CHECK(hipDeviceSynchronize());
    ALABI_HIP_CHECK(hipMemcpy(counts_host, e->nuts_counts, WT * 3 * sizeof(long long), hipMemcpyDeviceToHost));
    ALABI_HIP_CHECK(hipMemcpy(accept_host, e->nuts_accept, WT * sizeof(double), hipMemcpyDeviceToHost));
    if (reset) {
        ALABI_HIP_CHECK(hipMemset(e->nuts_counts, 0, WT * 3 * sizeof(long long)));
        ALABI_HIP_CHECK(hipMemset(e->nuts_accept, 0, WT * sizeof(double)));
    }
    return ALABI_OK;
}

int alabi_ens_step_with_randoms_nuts(alabi_ens* e, double* coords, double* logp, int k_move, double eps, const double* z0,
                                     const unsigned* dir, const double* u_leaf, const double* u_tree, int* trace, long long* n_accept,
                                     void* stream) {
    if (!e || !coords || !logp || !z0 || !dir || !u_leaf || !u_tree || e->E != 1 || !e->all_nuts) return ALABI_BAD_ARGUMENT;
    if (k_move < 0 || k_move >= e->moves.n || !(eps > 0.0) || !std::isfinite(eps)) return ALABI_BAD_ARGUMENT;
    if (!e->gp->computed || !e->gp->has_alpha) return ALABI_NOT_COMPUTED;
    hipStream_t s = as_stream(stream);
    const int st = ens_sync_consts(e, s);
    if (st != ALABI_OK) return st;
    const NutsInject inj{k_move, eps, z0, dir, u_leaf, u_tree, trace};
    return launch_ens_nuts(e, coords, logp, 0, 0, 1, 1, nullptr, nullptr, n_accept, &inj, s);
}

int alabi_ens_export_nuts_draws(alabi_ens* e, long long step, int max_depth, int* move, double* eps, double* z0, unsigned* dir,
                                double* u_leaf, double* u_tree, void* stream) {
    if (!e || !move || !eps || !z0 || !dir || !u_leaf || !u_tree || !e->all_nuts || max_depth < 1 || max_depth > ALABI_NUTS_MAX_DEPTH)
        return ALABI_BAD_ARGUMENT;
    return launch_ens_nuts_export(e, step, max_depth, move, eps, z0, dir, u_leaf, u_tree, as_stream(stream));
}

int alabi_ens_kde_singular(alabi_ens* e, long long* count) {
    if (!e || !count) return ALABI_BAD_ARGUMENT;
    *count = 0;
    if (!e->kde.singular) return ALABI_OK;
    unsigned long long v = 0;
    ALABI_HIP_CHECK(hipDeviceSynchronize());
    ALABI_HIP_CHECK(hipMemcpy(&v, e->kde.singular, sizeof(v), hipMemcpyDeviceToHost));
    *count = (long long)v;
    return ALABI_OK;
}

int alabi_ens_export_snooker_draws(alabi_ens* e, int* j3, void* stream) {
    if (!e || !j3 || e->drawn_n < 1 || !e->mv.cw3) return ALABI_BAD_ARGUMENT;
    ALABI_HIP_CHECK(hipMemcpyAsync(j3, e->mv.partner3, (size_t)e->W * e->E * sizeof(int), hipMemcpyDeviceToDevice, as_stream(stream)));
    return ALABI_OK;
}

int alabi_ens_export_partner_ids(alabi_ens* e, int* cw2, int* cw3, void* stream) {
    if (!e || e->drawn_n < 1 || (cw2 && !e->mv.cw2) || (cw3 && !e->mv.cw3)) return ALABI_BAD_ARGUMENT;
    const size_t bytes = (size_t)e->W * e->E * sizeof(int);
    if (cw2) ALABI_HIP_CHECK(hipMemcpyAsync(cw2, e->mv.cw2, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    if (cw3) ALABI_HIP_CHECK(hipMemcpyAsync(cw3, e->mv.cw3, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    return ALABI_OK;
}

int alabi_ens_export_move_draws(alabi_ens* e, int* move, int* j2, double* gamma, void* stream) {
    if (!e || !move || !j2 || !gamma || e->drawn_n < 1 || !e->mv.cw2) return ALABI_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    const size_t WT = (size_t)e->W * e->E;
    ALABI_HIP_CHECK(hipMemcpyAsync(move, e->mv.move, (size_t)e->E * sizeof(int), hipMemcpyDeviceToDevice, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(j2, e->mv.partner2, WT * sizeof(int), hipMemcpyDeviceToDevice, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(gamma, e->draws.zz, WT * sizeof(double), hipMemcpyDeviceToDevice, s));
    return ALABI_OK;
}

int alabi_ens_export_draws(alabi_ens* e, long long step, double a, int* order, int* n0, double* u_z, int* partner,
                           double* u_acc, int* cw, double* zz, void* stream) {
    if (!e || !order || !n0 || !u_z || !partner || !u_acc) return ALABI_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    int st;
    if ((st = alabi_ens_draw(e, step, 1, a, stream)) != ALABI_OK) return st;
    const size_t WT = (size_t)e->W * e->E;
    ALABI_HIP_CHECK(hipMemcpyAsync(order, e->draws.order, WT * sizeof(int), hipMemcpyDeviceToDevice, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(partner, e->draws.partner, WT * sizeof(int), hipMemcpyDeviceToDevice, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(u_z, e->draws.u_z, WT * sizeof(double), hipMemcpyDeviceToDevice, s));
    ALABI_HIP_CHECK(hipMemcpyAsync(u_acc, e->draws.u_acc, WT * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (cw) ALABI_HIP_CHECK(hipMemcpyAsync(cw, e->draws.cw, WT * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (zz) ALABI_HIP_CHECK(hipMemcpyAsync(zz, e->draws.zz, WT * sizeof(double), hipMemcpyDeviceToDevice, s));
    *n0 = (e->W + 1) / 2;
    return ALABI_OK;
}

}  // extern "C"
